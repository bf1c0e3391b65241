"""The width table of the diagonal statistics kernels (tests/em_width_cases.py) without a GPU: the conditions that make it a fair
yardstick for tests/test_gpu_em_widths.py and tests/test_gpu_bw_widths.py.  Every width the five lists of the sources name is met
by its smallest and its largest dim (so a width cannot be added without a row); the host code (tests/host/em_width_checks.cpp: the
plan, the padded dim, the packer) says of every row what the table expects -- the engine, the instantiation, and for the long rows
the tile loop, the uneven last chunk, the record ranges and the workgroups that return; every engine-3 start model is inside the
split-bf16 layout's range; and against the float64 oracle every mixture keeps at least two frames and a swap of two neighbouring
dimensions moves the answer by at least a hundred gates."""
import math
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bw_cases as bc  # noqa: E402
import em_width_cases as wc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
GROUPS = wc.groups()


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(text):
    return [int(v) for v in re.findall(r"\d+", text)]


def test_table_is_the_one_written_down():
    assert wc.ENGINE1_DIMS == [1, 8, 9, 13, 14, 16, 17, 24, 25, 26, 27, 32, 33, 34, 35, 39, 40, 41, 48, 49, 56, 57, 64, 65, 80, 81, 96]
    assert wc.ENGINE2_DIMS == [1, 8, 9, 13, 14, 16, 17, 24, 25, 26, 27, 32, 33, 34, 35, 39, 40]
    assert wc.SPLIT_DIMS == {(8, 1): [1, 7], (8, 2): [8], (13, 2): [9, 13], (16, 2): [14, 15], (16, 3): [16], (24, 3): [17, 23], (24, 4): [24],
                             (26, 4): [25, 26], (32, 4): [27, 31], (32, 5): [32], (34, 5): [33, 34], (39, 5): [35, 39]}
    assert [wc.padded(d) for d in wc.WIDE_DIMS] == [128, 128, 192]
    rows = wc.rows()
    assert len(set(rows)) == len(rows) and len(set(wc.LONG_ROWS)) == len(wc.LONG_ROWS)
    # 27 + 3 dims of engine 1; 17 dims and 9 widths x 3 of engine 2; 20 dims and 12 shapes x 3 of engine 3; D = 40 under option 3
    assert len(rows) == 30 + 17 + 27 + 20 + 36 + 1
    assert len(GROUPS) == 15 + 9 + 12 + 1 + len(wc.LONG_ROWS) and sum(len(rs) for _, rs in GROUPS) == len(rows) + len(wc.LONG_ROWS)
    # K = 70: 18 records, the last with two dead mixtures; two workgroups of 64, the second with 6 live.  n = 300: 2 x 128 + 44 = 256 + 44
    assert -(-wc.BASE_K // 4) == 18 and 18 * 4 - wc.BASE_K == 2 and wc.BASE_K - 64 == 6 and wc.BASE_N == 2 * 128 + 44
    # the split layout's base shape: three tiles of one workgroup, at most a quarter padding, the last tile and the last record ragged
    assert -(-wc.SPLIT_K // 32) == 3 and 1.0 - wc.SPLIT_K / 96.0 <= wc.MFMA_MAX_PAD_WASTE < 1.0 - (wc.BASE_K) / 96.0
    assert wc.SPLIT_K % 32 == 9 and wc.SPLIT_K % 4 == 1 and 1.0 - (wc.SPLIT_K - 2) / 96.0 > wc.MFMA_MAX_PAD_WASTE
    assert 1.0 - wc.FEW_K[3] / 32.0 <= wc.MFMA_MAX_PAD_WASTE < 1.0 - (wc.FEW_K[3] - 1) / 32.0
    assert wc.MANY_K == {2: 2 * 64 + 1, 3: 128 + 32}
    # what the mixed blocks hold: REM = 0 at 16 and 32 (the count alone); 2 REM + 1 = 17 at 8, 24, 40 (the count alone in a second
    # mixed block); REM = 2 at 34; x and x^2 across the block border at 13 and 26
    assert [dp for dp in wc.MFMA_DPS if dp % 16 == 0] == [16, 32] and [dp for dp in wc.MFMA_DPS if 2 * (dp % 16) + 1 == 17] == [8, 24, 40]
    assert [wc.emm_ncb(dp) - 2 * (dp // 16) for dp in wc.MFMA_DPS] == [2, 2, 1, 2, 2, 1, 1, 1, 2]
    # Baum-Welch: with D = 1, 13, 39, 40 of tests/test_gpu_bw_stats.py both ends of every width; the widths it never ran, whole
    assert {wc.padded(d) for d in wc.BW_DIMS} == set(wc.MFMA_DPS) - {40} and not set(wc.BW_DIMS) & {1, 13, 39, 40}
    for dp in (16, 24, 26, 32, 34):
        assert set(wc.MFMA_DIMS[dp]) <= set(wc.BW_DIMS), dp
    assert {8, 9, 14} <= set(wc.BW_DIMS) and wc.BW_RAGGED == (0, 1, 3, 63, 64, 65, 127, 128, 129, 259) and wc.BW_R == 128


def test_every_built_width_has_its_rows():
    shapes = _source("em_shapes.hpp")
    vector = _ints(re.search(r"#define SR_EM_VECTOR_DPS\(X\)(.*)", shapes).group(1))
    mfma = _ints(re.search(r"#define SR_EM_MFMA_DPS\(X\)(.*)", shapes).group(1))
    split = [(int(a), int(b)) for a, b in re.findall(r"X\((\d+), *(\d+)\)", re.search(r"#define SR_EM_SPLIT_SHAPES\(X\)(.*)", shapes).group(1))]
    bw = _ints(re.search(r"#define SR_BW_DIMS\(CASE\)(.*)", _source("bw_stats.hip")).group(1))
    kdims = _ints(re.search(r"kDims\[\] = \{([^}]*)\}", _source("model_pack.cpp")).group(1))
    bw_restated = _ints(re.search(r"static const int dims\[\] = \{([^}]*)\}", _source("bw_plan.cpp")).group(1))
    bw_max = int(re.search(r"BW_MAX_DIM = (\d+)", _source("bw_plan.hpp")).group(1))
    assert int(re.search(r"WIDE_DC = (\d+)", _source("model_pack.hpp")).group(1)) == wc.WIDE_DC
    assert (vector, mfma, split, kdims) == (wc.KDIMS, wc.MFMA_DPS, wc.SPLIT_SHAPES, wc.KDIMS)
    assert bw == wc.MFMA_DPS and bw_restated == [d for d in kdims if d <= bw_max] == bw and bw_max == bw[-1]
    # both ends of every instantiation, found with the SOURCES' lists, are rows; no row maps to a width that is not built

    def pad(dim):
        return next(d for d in kdims if d >= dim)

    have = {e: {(r.dim) for r in wc.rows() if r.engine == e and r.option == e and r.K in (wc.BASE_K, wc.SPLIT_K) and r.kind == "em"} for e in (1, 2, 3)}
    for dp in vector:
        dims = [d for d in range(1, kdims[-1] + 1) if pad(d) == dp]
        assert dims and {dims[0], dims[-1]} <= have[1], dp
    for dp in mfma:
        dims = [d for d in range(1, mfma[-1] + 1) if pad(d) == dp]
        assert dims and {dims[0], dims[-1]} <= have[2], dp
    for dp, ks in split:
        dims = [d for d in range(1, mfma[-1] + 1) if (pad(d), (d + 8) // 8) == (dp, ks)]
        assert dims and {dims[0], dims[-1]} <= have[3], (dp, ks)
    for dp in bw:
        dims = [d for d in range(1, bw_max + 1) if pad(d) == dp]
        assert {dims[0], dims[-1]} <= set(wc.BW_DIMS) | {1, 13, 39, 40}, dp              # (those four: tests/test_gpu_bw_stats.py)
    for r in wc.rows() + wc.LONG_ROWS + wc.twin_rows():
        dp = wc.padded(r.dim)
        assert (dp in vector or dp % wc.WIDE_DC == 0) if r.engine == 1 else dp in mfma if r.engine == 2 else (dp, wc.ks_of(r.dim)) in split, r
    assert all(wc.padded(d) in bw for d in wc.BW_DIMS + wc.BW_LONG_DIMS + wc.BW_RESIDENT_DIMS)
    # the extra shapes, the MAP row and the twin row sit at the largest dim of every width
    for e, ends in ((2, wc.MFMA_DIMS), (3, wc.SPLIT_DIMS)):
        for width, dims in ends.items():
            at = [r for r in wc.rows() if r.option == e and r.engine == e and wc.width_of(r) == width and r.dim == dims[-1]]
            assert sorted((r.K, r.n, r.kind) for r in at) == sorted([(wc.SPLIT_K if e == 3 else wc.BASE_K, wc.BASE_N, "em"), (wc.FEW_K[e], wc.FEW_N, "em"),
                                                                    (wc.MANY_K[e], wc.MANY_N, "em"), (wc.SPLIT_K if e == 3 else wc.BASE_K, wc.BASE_N, "map")]), (e, width)
    assert [r.dim for r in wc.twin_rows()] == [wc.SPLIT_DIMS[s][-1] for s in wc.SPLIT_SHAPES]


@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    """tests/host/em_width_checks.cpp on every row: {row: its line as a dict}"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    tmp = tmp_path_factory.mktemp("em_width")
    exe = str(tmp / "em_width_checks")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O1", "-std=c++17", "-I", CSRC, "-I", os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "host", "em_width_checks.cpp")] + \
          [os.path.join(CSRC, s) for s in ("em_plan.cpp", "map_plan.cpp", "model_pack.cpp", "fp_parts.cpp")] + ["-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    rows = wc.rows() + wc.twin_rows() + wc.LONG_ROWS
    path = str(tmp / "rows.bin")
    with open(path, "wb") as f:
        for r in rows:
            with_model = r.option == 3
            f.write(struct.pack("<4iq", r.option, r.dim, r.K, int(with_model), r.n))
            if with_model:
                for a in wc.make_data(r.dim, r.K, r.n)[2]:
                    f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    names = "option dim K n dp engine ks grid_x grid_y block n_tiles wg_mix ncb wide amp pad_waste in_range".split()
    lines = [dict(zip(names, (float(v) if "." in v or "e" in v else int(v) for v in line.split()))) for line in r.stdout.strip().split("\n")]
    assert len(lines) == len(rows)
    for row, ln in zip(rows, lines):
        assert (ln["option"], ln["dim"], ln["K"], ln["n"]) == (row.option, row.dim, row.K, row.n)
    return dict(zip(rows, lines))


def test_host_code_agrees_with_the_table(host_lines):
    for row, ln in host_lines.items():
        assert ln["engine"] == row.engine and ln["dp"] == wc.padded(row.dim), (row, ln)
        assert ln["ks"] == (wc.ks_of(row.dim) if row.engine == 3 else 0), (row, ln)
        assert ln["wide"] == (wc.padded(row.dim) > wc.KDIMS[-1]) and ln["wg_mix"] == {1: 0, 2: 64, 3: 128}[row.engine], (row, ln)
        if row.engine != 1:
            assert ln["ncb"] == wc.emm_ncb(ln["dp"]) and ln["n_tiles"] == -(-row.n // 128), (row, ln)
            assert ln["grid_x"] == (-(-row.K // 128) if row.engine == 3 else -(-row.K // 64)), (row, ln)
    # K = 70 / 73 at n = 300: two (engine 2) or one (engine 3) workgroup column, three tiles, one each
    for row, ln in host_lines.items():
        if row.K in (wc.BASE_K, wc.SPLIT_K) and row.engine != 1 and row not in wc.LONG_ROWS:
            assert (ln["grid_x"], ln["grid_y"], ln["n_tiles"]) == (2 if row.engine == 2 else 1, 3, 3), (row, ln)


def test_engine_3_start_models_are_inside_the_split_layouts_range(host_lines):
    worst_amp, worst_waste = 0.0, 0.0
    for row, ln in host_lines.items():
        if row.option != 3:
            continue
        assert ln["in_range"] == 1 and ln["amp"] <= wc.MFMA_MAX_AMP and ln["pad_waste"] <= wc.MFMA_MAX_PAD_WASTE, (row, ln)
        worst_amp, worst_waste = max(worst_amp, ln["amp"]), max(worst_waste, ln["pad_waste"])
    print("engine-3 start models: largest amp %.0f (bound %.0f), largest padding waste %.3f (bound %.2f)"
          % (worst_amp, wc.MFMA_MAX_AMP, worst_waste, wc.MFMA_MAX_PAD_WASTE))
    # K = 70 would not be: the plan hands it to engine 2
    assert 1.0 - wc.BASE_K / 96.0 > wc.MFMA_MAX_PAD_WASTE


def test_long_rows_walk_what_they_are_for(host_lines):
    for row in wc.LONG_ROWS:
        ln = host_lines[row]
        if row.engine in (2, 3):
            tiles_per = -(-ln["n_tiles"] // ln["grid_y"])
            used = -(-ln["n_tiles"] // tiles_per)
            last = ln["n_tiles"] - (used - 1) * tiles_per
            print("%s: %d tiles over %d chunks: %d a chunk, %d chunks with tiles, the last with %d" % (row, ln["n_tiles"], ln["grid_y"], tiles_per, used, last))
            assert tiles_per >= 2 and 1 <= last < tiles_per and used <= ln["grid_y"], (row, ln)
            assert row.n % 128 != 0                                   # and a ragged last tile
        else:
            n_records = -(-row.K // 4)
            rec_per = -(-n_records // ln["grid_y"])
            used = -(-n_records // rec_per)
            print("%s: %d tiles on gridDim.x = %d; %d records over gridDim.y = %d: %d a workgroup, %d without records"
                  % (row, ln["n_tiles"], ln["grid_x"], n_records, ln["grid_y"], rec_per, ln["grid_y"] - used))
            assert ln["n_tiles"] == -(-row.n // 256) and row.n % 256 != 0
            if row.K == 68:
                assert rec_per >= 2 and used < ln["grid_y"] and ln["n_tiles"] == ln["grid_x"], (row, ln)
            else:
                assert ln["n_tiles"] > ln["grid_x"] and rec_per >= 2, (row, ln)            # the tile loop's stride
    assert sorted((r.engine, r.dim) for r in wc.LONG_ROWS if r.K != 8) == [(e, d) for e in (1, 2, 3) for d in (13, 32)]
    assert wc.emm_ncb(13) - 0 == 2 and 32 % 16 == 0                  # two mixed blocks; REM = 0


@pytest.mark.parametrize("gid,rows", GROUPS, ids=[g for g, _ in GROUPS])
def test_rows_are_well_posed_and_show_a_wrong_column(oracle_built, gid, rows):
    """Every mixture keeps MIN_OCCUPANCY frames after the iteration: the device's fp32 posteriors decide nothing and no mixture's
    sums are redone on the host.  Swapping two neighbouring dimensions of the oracle's means, or of its sigmas, moves some mixture
    by SWAP_MARGIN gates: a column mix-up cannot pass."""
    for row in rows + [t for t in wc.twin_rows() if t._replace(option=3, engine=3) in rows]:
        cent, X, start = wc.make_data(row.dim, row.K, row.n)
        assert X.dtype == np.float32 and X.shape == (row.n, row.dim) and start[1].shape == (row.K, row.dim)
        assert np.array_equal(start[1], np.vectorize(lambda v: float("%g" % v))(start[1]))
        w, mu, sg, occ = wc.oracle_iteration(oracle_built, row)
        m_mu, m_sg = wc.swap_margins(mu, sg)
        print("%s: smallest occupancy %.2f frames; a swap of neighbouring dimensions moves the means by >= %.0f gates, the sigmas by >= %.0f"
              % (row, occ.min(), m_mu, m_sg))
        assert occ.min() >= wc.MIN_OCCUPANCY, (row, float(occ.min()))
        assert m_mu >= wc.SWAP_MARGIN, (row, m_mu)
        if row.kind == "em":
            assert m_sg >= wc.SWAP_MARGIN, (row, m_sg)
        else:
            assert np.array_equal(w, start[0]) and np.array_equal(sg, start[2])       # MAP: means only


@pytest.mark.parametrize("D", wc.BW_DIMS)
def test_baum_welch_rows_show_a_wrong_column(D):
    """Neighbouring dimensions of every mixture's F differ by far more than the F gate, in some utterance of the row."""
    for K in wc.BW_KS:
        ubm, utts = wc.bw_case(bc, K, D)
        m = wc.bw_swap_margin(bc.batch_stats(utts, ubm), K, D)
        print("Baum-Welch K=%d D=%d: neighbouring dimensions of F differ by >= %.0f gates in every mixture" % (K, D, m))
        assert m >= wc.SWAP_MARGIN, (K, D, m)
    if D in wc.BW_LONG_DIMS:
        ubm, utts = wc.bw_long_case(bc, D)
        m = wc.bw_swap_margin(bc.batch_stats(utts, ubm), wc.BW_LONG_K, D)
        print("Baum-Welch K=%d D=%d, %d frames: >= %.0f gates" % (wc.BW_LONG_K, D, wc.BW_LONG_T, m))
        assert m >= wc.SWAP_MARGIN and math.ceil(wc.BW_LONG_T / 128) == 9 and wc.BW_LONG_T > 1024, (D, m)
