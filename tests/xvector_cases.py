"""The x-vector forward pass's checker, shared by tests/test_xvector_cpu.py and tests/test_gpu_xvector.py: a numpy restatement of the
arithmetic contract (include/pygmm_hip.h, "Speaker embeddings"), the gates, the case tables and the mutants.

Restatement: weights and stored activations are rounded to bf16, round to nearest even, on the integer bits; a layer accumulates in
float64; y = scale * act(W x_ctx + b) + shift; the pooling is mean and sqrt(max(E[x^2] - mean^2, var_floor)) in float64.

Layer gate (derived, not tuned).  For a layer fed the device's own input let `a` be the restatement's float64 value before the store
is rounded, K = m C_in the length of the sum, and
    beta = |scale| * c * (K + 2) * 2^-24 * (sum |w| |x| + |b|)  +  2 ulp32(a).
The first term bounds an fp32 accumulation of K products and the bias in any order and under either rounding of the partial sums
(the bias is the sum's last term, hence it stands in the sum of magnitudes; the products of bf16 values are exact in fp32); the second
the epilogue's two roundings.  c = 2: the round-toward-zero worst case.  Nothing on this project's shelf establishes that the bf16
MFMA rounds to nearest inside and between its K steps, so the weaker assumption is the one used.
fp32 store: |y_dev - a| <= beta.  bf16 store: RNE(a - beta) <= y_dev <= RNE(a + beta) -- rounding is monotone, so this admits a
boundary flip only where one is possible.

Pooling gate: float64 sums of n terms: |mean_dev - mean| <= n 2^-53 sum|x| / n (+ the fp32 store's half ulp); the standard deviation
gets the same bound on E2 pushed through E2 - m^2 and the square root, i.e. a relative bound amplified by E2 / var; `POOL_AMP_MAX` is
the ceiling on E2 / var that the CPU test asserts on every pooling input, so that the gate stays below 1e-6 relative.

Mutants (each must fall outside the gate on the GPU tests' own inputs; asserted on the CPU): see MUTANTS.
"""
import numpy as np

C_GATE = 2.0
POOL_AMP_MAX = 1e6
STD_NETWORK = ((30, 512, (-2, -1, 0, 1, 2)), (512, 512, (-2, 0, 2)), (512, 512, (-3, 0, 3)), (512, 512, (0,)), (512, 1500, (0,)))
STD_EMBED = 512
K_STAGE = 64          # the kernel's K per stage: what the "bias per K chunk" mutant repeats the bias over


# ---- bf16 on the integer bits ----

def bf16_rne(x):
    """float32 values rounded to bf16, round to nearest even; returned as float32 (the low 16 bits are zero)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    r = np.where(nan, ((u >> 16) | 0x40) << 16, r)
    return (r & 0xffffffff).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_trunc(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xffff0000)).view(np.float32).reshape(np.shape(x))


def rne32_from64(a):
    """float64 -> the nearest float32 (numpy's cast rounds to nearest even)."""
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def bf16_from64(a):
    """float64 -> bf16 (as float32), round to nearest even in ONE step (through float32 a value could round twice): a bf16 keeps 8
    significant bits, so with a = m 2^e, 0.5 <= |m| < 1, the result is rint(256 m) 2^(e - 8) -- numpy's rint rounds ties to even.
    (bf16 subnormals, below 2^-126, do not occur in the tests: 0 stays 0.)"""
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8).astype(np.float32)


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- the layers ----

def make_layer(rng, kind, c_in, c_out, offsets=(0,), act="relu", affine=True):
    m = len(offsets)
    W = (rng.standard_normal((c_out, m * c_in)) / np.sqrt(m * c_in)).astype(np.float32)
    b = (0.1 * rng.standard_normal(c_out)).astype(np.float32)
    l = {"kind": kind, "offsets": tuple(offsets), "W": W, "b": b, "act": act, "scale": None, "shift": None}
    if affine:
        l["scale"] = (0.5 + rng.random(c_out)).astype(np.float32)
        l["shift"] = (0.1 * rng.standard_normal(c_out)).astype(np.float32)
    return l


def pool_layer(channels, var_floor=1e-10):
    return {"kind": "stats_pool", "channels": int(channels), "var_floor": float(var_floor)}


def standard_network(seed=28):
    rng = np.random.default_rng(seed)
    layers = [make_layer(rng, "tdnn", ci, co, off) for ci, co, off in STD_NETWORK]
    # (floor 1e-6, not the default 1e-10: behind a ReLU some of 1500 random channels fire a few times in hundreds of frames, and a
    # variance of 3e-10 beside E2 = 1e-3 would put E2 / var above POOL_AMP_MAX, the condition the pooling gate rests on)
    layers.append(pool_layer(1500, var_floor=1e-6))
    layers.append(make_layer(rng, "affine", 3000, STD_EMBED, act="none", affine=False))
    return layers


def irregular_network(seed=29):
    """widths 24 -> 33 -> 200 -> 31, pooling, 17"""
    rng = np.random.default_rng(seed)
    return [make_layer(rng, "tdnn", 24, 33, (-1, 0, 2)), make_layer(rng, "tdnn", 33, 200, (0, 4), affine=False),
            make_layer(rng, "tdnn", 200, 31, (-5,), act="none"), pool_layer(31), make_layer(rng, "affine", 62, 17, act="none")]


def single_layer_network(rng, c_in, c_out, offsets, act="relu", affine=True):
    """the layer under test, a pooling and a small embedding layer behind it"""
    return [make_layer(rng, "tdnn", c_in, c_out, offsets, act, affine), pool_layer(c_out), make_layer(rng, "affine", 2 * c_out, 4, act="none", affine=False)]


def context_of(layers):
    return sum(l["offsets"][-1] - l["offsets"][0] for l in layers if l["kind"] == "tdnn")


def layer_forward(layer, X, mutant=None):
    """X: float64 [T, C_in], the layer's (bf16-valued) input of ONE segment.  -> (a, S): the float64 output before the store is
    rounded, and sum |w| |x| + |b| per output element."""
    X = np.asarray(X, dtype=np.float64)
    off = list(layer["offsets"])
    m, span = len(off), off[-1] - off[0]
    T_out = X.shape[0] - span
    Wq = bf16_rne(layer["W"]).astype(np.float64)
    if mutant == "exact_weights":          # (no mutant of the device's: the unrounded network of network_forward)
        Wq = layer["W"].astype(np.float64)
    b = layer["b"].astype(np.float64)
    shifts = [o - off[0] for o in off]
    if mutant == "offsets_reversed":
        shifts = shifts[::-1]
    if mutant == "off_by_one":
        shifts = [s + 1 for s in shifts]
        X = np.concatenate([X, X[-1:]], axis=0)
    Xc = np.concatenate([X[s:s + T_out] for s in shifts], axis=1)
    acc = Xc @ Wq.T
    S = np.abs(Xc) @ np.abs(Wq).T + np.abs(b)
    z = acc + b
    if mutant == "bias_per_chunk":
        c_pad = -(-X.shape[1] // 32) * 32
        z = acc + b * (-(-(m * c_pad) // K_STAGE))
    relu = layer["act"] == "relu"
    sc = np.ones_like(b) if layer["scale"] is None else layer["scale"].astype(np.float64)
    sh = np.zeros_like(b) if layer["shift"] is None else layer["shift"].astype(np.float64)
    if mutant == "affine_before_relu":
        a = sc * z + sh
        return (np.maximum(a, 0.0) if relu else a), S
    a = np.maximum(z, 0.0) if relu else z
    return sc * a + sh, S


def layer_beta(layer, a, S):
    K = layer["W"].shape[1]
    sc = 1.0 if layer["scale"] is None else np.abs(layer["scale"].astype(np.float64))
    return sc * C_GATE * (K + 2) * 2.0 ** -24 * S + 2.0 * ulp32(a)


def layer_gate_f32(layer, a, S, y_dev):
    """worst |y_dev - a| / beta over the elements (<= 1 passes)"""
    beta = layer_beta(layer, a, S)
    return float(np.max(np.abs(np.asarray(y_dev, dtype=np.float64) - a) / beta)) if a.size else 0.0


def layer_gate_bf16(layer, a, S, y_dev):
    """number of elements outside [RNE(a - beta), RNE(a + beta)]"""
    beta = layer_beta(layer, a, S)
    lo, hi = bf16_from64(a - beta), bf16_from64(a + beta)
    y = np.asarray(y_dev, dtype=np.float32)
    return int(np.sum((y < lo) | (y > hi)))


def pool_forward(layer, X, mutant=None):
    """X: float64 [n, C] of one segment -> float64 [2 C]"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    mean = X.sum(axis=0) / n
    e2 = (X * X).sum(axis=0) / n
    var = e2 - mean * mean
    if mutant == "n_minus_1":
        var = var * n / max(n - 1, 1)
    if mutant == "floor_on_std":
        std = np.maximum(np.sqrt(np.maximum(var, 0.0)), layer["var_floor"])
    else:
        std = np.sqrt(np.maximum(var, layer["var_floor"]))
    return np.concatenate([std, mean]) if mutant == "std_mean_order" else np.concatenate([mean, std])


def pool_gate(layer, X, y_dev):
    """worst error / bound over [mean | std] (<= 1 passes) and the largest E2 / var among the channels the floor does not take"""
    X = np.asarray(X, dtype=np.float64)
    n, C = X.shape
    want = pool_forward(layer, X)
    mean, std = want[:C], want[C:]
    e_mean = n * 2.0 ** -53 * np.abs(X).sum(axis=0) / n
    e2 = (X * X).sum(axis=0) / n
    var = e2 - mean * mean
    floored = var <= layer["var_floor"]
    # d(var) <= d(E2) + 2 |m| d(m); d(std) = d(var) / (2 std); a floored channel's std is exact up to the store
    e_var = n * 2.0 ** -53 * e2 + 2.0 * np.abs(mean) * e_mean
    e_std = np.where(floored, 0.0, e_var / (2.0 * np.maximum(std, 1e-300)))
    bound = np.concatenate([e_mean, e_std]) + 0.5 * ulp32(want) + 1e-300
    y = np.asarray(y_dev, dtype=np.float64)
    amp = float(np.max(np.where(floored, 0.0, e2 / np.maximum(var, 1e-300)))) if C else 0.0
    return float(np.max(np.abs(y - want) / bound)), amp


def network_forward(layers, X, rounded=True):
    """One segment through the whole network: `rounded` follows the contract (bf16 inputs, weights and stored activations); without
    it the unrounded float64 network (what bf16 costs is the distance between the two)."""
    x = bf16_rne(X).astype(np.float64) if rounded else np.asarray(X, dtype=np.float64)
    for i, l in enumerate(layers):
        if l["kind"] == "stats_pool":
            x = pool_forward(l, x)[None, :]
            if rounded:
                x = bf16_rne(rne32_from64(x)).astype(np.float64)
            continue
        a, _ = layer_forward(l, x, mutant=None if rounded else "exact_weights")
        last = i == len(layers) - 1
        x = a if (last or not rounded) else bf16_from64(a).astype(np.float64)
    return x[0]


MUTANTS_LAYER = ("offsets_reversed", "off_by_one", "affine_before_relu", "bias_per_chunk")
MUTANTS_POOL = ("n_minus_1", "std_mean_order", "floor_on_std")
MUTANTS = MUTANTS_LAYER + ("store_truncated",) + MUTANTS_POOL


# ---- the case tables (TM, TN: the kernel's tile, from the plan) ----

C_IN = (1, 24, 31, 32, 33, 39, 160)
OFFSETS = ((0,), (-2, -1, 0, 1, 2), (-3, 0, 3), (-1, 0, 2), (0, 4), (-5,))


def c_out_values(TN):
    return (1, 31, 33, TN - 1, TN, TN + 1, 200)


def layer_cases(TN):
    """A covering subset of C_in x C_out x offsets: case i pairs C_in[i] with C_out[3 i mod 7] and offsets[i mod 6] -- every value of
    every axis appears (7 and 3 are coprime; i = 0 .. 6 covers the six offset sets) -- plus (-3, 0, 3) x 512, whose K spans 24
    stages.  Case 0 (C_in = 1, one offset) has a K shorter than a stage.  Odd cases carry scale / shift, cases 2 and 5 no ReLU."""
    co = c_out_values(TN)
    cases = [(C_IN[i], co[(3 * i) % 7], OFFSETS[i % 6], "none" if i in (2, 5) else "relu", i % 2 == 1) for i in range(7)]
    cases.append((512, 33, (-3, 0, 3), "relu", True))
    return cases


def row_edge_rows(TM):
    return (1, TM - 1, TM, TM + 1, 2 * TM + 3)


POOL_N = (1, 2, 63, 64, 65, 1000)
POOL_C = (1, 33, 1500)


def pool_input(n, C, seed=5):
    """fp32 features for the pooling cases: channel 0 is constant (the variance floor is taken there), the others N(0.3, 1)"""
    rng = np.random.default_rng(seed + 1000 * n + C)
    X = (0.3 + rng.standard_normal((n, C))).astype(np.float32)
    X[:, 0] = 1.25
    return X


def pooling_input(layers, X):
    """the restatement's input of the pooling layer for one segment's features: what the CPU test checks the gate's condition on"""
    x = bf16_rne(X).astype(np.float64)
    for l in layers:
        if l["kind"] == "stats_pool":
            return l, x
        a, _ = layer_forward(l, x)
        x = bf16_from64(a).astype(np.float64)
    raise ValueError("no stats_pool")


STD_TEST_FRAMES, STD_TEST_SEED = (15, 200, 457), 3
IRR_TEST_FRAMES, IRR_TEST_SEED = (8, 9, 150, 300), 4


def network_test_features(frames, seed, D):
    rng = np.random.default_rng(seed)
    return [features(rng, T, D) for T in frames]


def features(rng, T, D):
    return rng.standard_normal((T, D)).astype(np.float32)


def mutant_layer_case(TN):
    """the single-layer case the layer mutants are run on: irregular offsets, scale / shift and a ReLU"""
    rng = np.random.default_rng(77)
    net = single_layer_network(rng, 33, TN + 1, (-1, 0, 2), "relu", True)
    X = features(rng, 40, 33)
    return net, X
