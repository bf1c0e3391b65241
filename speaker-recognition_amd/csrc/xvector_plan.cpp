// xvector_plan.cpp -- the x-vector forward pass's plan (xvector_plan.hpp): pure host code.
#include "xvector_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace sr {

namespace {

std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    char buf[512];
    std::snprintf(buf, sizeof buf, f, a, b, c, d);
    return buf;
}

int round_up(int v, int g) { return (v + g - 1) / g * g; }

}  // namespace

XvLayer xv_layer_from_desc(const int32_t *d, double var_floor) {
    XvLayer L;
    L.kind = d[0];
    L.c_in = d[1];
    L.c_out = d[2];
    L.act = d[3];
    L.has_affine = d[4] != 0;
    L.n_off = d[5];
    for (int j = 0; j < XV_MAX_OFFSETS; j++) L.off[j] = d[6 + j];
    L.var_floor = var_floor;
    return L;
}

bool xv_check_model(const XvLayer *layers, int n_layers, XvModelInfo &m, std::string &why) {
    m = XvModelInfo();
    if (!layers || n_layers < 2 || n_layers > XV_MAX_LAYERS) {
        why = fmt("%lld layers; a network holds 2 .. %lld (a stats_pool and at least one affine layer after it)", n_layers, XV_MAX_LAYERS);
        return false;
    }
    m.n_layers = n_layers;
    int n_pool = 0;
    for (int l = 0; l < n_layers; l++) {
        const XvLayer &L = layers[l];
        if (L.kind != XV_TDNN && L.kind != XV_POOL && L.kind != XV_AFFINE) {
            why = fmt("layer %lld: kind %lld; 0 (tdnn), 1 (stats_pool) or 2 (affine)", l, L.kind);
            return false;
        }
        if (L.kind == XV_POOL) {
            n_pool++;
            if (n_pool == 1) m.pool = l;
        }
    }
    if (n_pool != 1) {
        why = fmt("%lld stats_pool layers; a network holds exactly one, between its frame layers and its segment layers", n_pool);
        return false;
    }
    if (m.pool == n_layers - 1) {
        why = "the network ends at its stats_pool; at least one affine layer follows it (the embedding layer)";
        return false;
    }
    m.width.resize((size_t)n_layers + 1);
    m.span.assign((size_t)n_layers, 0);
    for (int l = 0; l < n_layers; l++) {
        const XvLayer &L = layers[l];
        if (l < m.pool && L.kind != XV_TDNN) {
            why = fmt("layer %lld is affine in front of the stats_pool; frame layers are tdnn (offsets (0,) for a per-frame affine)", l);
            return false;
        }
        if (l > m.pool && L.kind != XV_AFFINE) {
            why = fmt("layer %lld is a tdnn behind the stats_pool; segment layers are affine", l);
            return false;
        }
        if (L.c_in < 1 || L.c_in > XV_MAX_C) {
            why = fmt("layer %lld: %lld input channels; 1 .. %lld", l, L.c_in, XV_MAX_C);
            return false;
        }
        const int want_out = L.kind == XV_POOL ? 2 * L.c_in : L.c_out;
        if (want_out < 1 || want_out > XV_MAX_C) {
            why = fmt("layer %lld: %lld output channels; 1 .. %lld (a stats_pool doubles its input's)", l, want_out, XV_MAX_C);
            return false;
        }
        if (l > 0 && L.c_in != m.width[(size_t)l]) {
            why = fmt("layer %lld takes %lld channels, layer %lld gives %lld; consecutive layers must agree", l, L.c_in, l - 1, m.width[(size_t)l]);
            return false;
        }
        m.width[(size_t)l] = L.c_in;
        m.width[(size_t)l + 1] = want_out;
        if (L.kind == XV_POOL) {
            if (!(L.var_floor >= 0.0) || !(L.var_floor < 1e300)) {
                why = fmt("layer %lld: the variance floor must be finite and >= 0", l);
                return false;
            }
            continue;
        }
        if (L.act != XV_ACT_NONE && L.act != XV_ACT_RELU) {
            why = fmt("layer %lld: act %lld; 0 (none) or 1 (relu)", l, L.act);
            return false;
        }
        if (L.kind == XV_AFFINE) {
            if (L.n_off != 1 || L.off[0] != 0) {
                why = fmt("layer %lld: an affine layer has the single offset 0", l);
                return false;
            }
            continue;
        }
        if (L.n_off < 1 || L.n_off > XV_MAX_OFFSETS) {
            why = fmt("layer %lld: %lld offsets; 1 .. %lld", l, L.n_off, XV_MAX_OFFSETS);
            return false;
        }
        for (int j = 0; j < L.n_off; j++) {
            if (L.off[j] < -XV_MAX_OFFSET || L.off[j] > XV_MAX_OFFSET) {
                why = fmt("layer %lld: offset %lld; within -%lld .. %lld", l, L.off[j], XV_MAX_OFFSET, XV_MAX_OFFSET);
                return false;
            }
            if (j > 0 && L.off[j] <= L.off[j - 1]) {
                why = fmt("layer %lld: offsets must ascend strictly (%lld follows %lld); sort them and reorder the blocks of W with them", l, L.off[j],
                          L.off[j - 1]);
                return false;
            }
        }
        m.span[(size_t)l] = L.off[L.n_off - 1] - L.off[0];
        m.context += m.span[(size_t)l];
    }
    if (layers[n_layers - 1].act != XV_ACT_NONE) {
        why = fmt("the last layer's act must be none: cut the network at the embedding layer's affine output (layer %lld has relu)", n_layers - 1);
        return false;
    }
    m.input_dim = m.width[0];
    m.embedding_dim = m.width[(size_t)n_layers];
    m.width_pad.resize(m.width.size());
    for (size_t s = 0; s < m.width.size(); s++) m.width_pad[s] = round_up(m.width[s], XV_GRAN);
    m.k_pad.assign((size_t)n_layers, 0);
    m.n_pad.assign((size_t)n_layers, 0);
    for (int l = 0; l < n_layers; l++) {
        if (layers[l].kind == XV_POOL) continue;
        m.k_pad[(size_t)l] = round_up(layers[l].n_off * m.width_pad[(size_t)l], XV_KC);
        m.n_pad[(size_t)l] = round_up(layers[l].c_out, XV_TN);
    }
    return true;
}

int64_t xv_segment_bytes(const XvModelInfo &m, int64_t n_frames, int last, bool tap_bf16) {
    // frame-level stages held as bf16: 0 .. pool, or 0 .. last (+ 1 when the tapped layer stores bf16)
    const int top_stage = last >= m.pool ? m.pool : (tap_bf16 ? last + 1 : last);
    int64_t a = 0, b = 0;      // the largest and the second largest
    for (int s = 0; s <= top_stage; s++) {
        const int64_t v = xv_stage_rows(m, n_frames, s) * m.width_pad[(size_t)s] * 2;
        if (v > a) {
            b = a;
            a = v;
        } else if (v > b) {
            b = v;
        }
    }
    int64_t total = a + b;
    if (last < m.pool) {
        if (!tap_bf16) total += xv_stage_rows(m, n_frames, last + 1) * m.width[(size_t)last + 1] * 4;
    } else {
        for (int s = m.pool + 1; s <= last + 1; s++) total += (int64_t)m.width_pad[(size_t)s] * 6;      // fp32 as written, bf16 as read
    }
    return total;
}

bool plan_xvector(const XvLayer *layers, int n_layers, const int64_t *lengths, int64_t n_seg, int tap, bool tap_bf16, int64_t scratch_bytes,
                  XvPlan &p, std::string &why) {
    p = XvPlan();
    if (!xv_check_model(layers, n_layers, p.info, why)) return false;
    const XvModelInfo &m = p.info;
    if (tap < -1 || tap >= n_layers) {
        why = fmt("tap %lld; -1 (the embedding) or a layer 0 .. %lld", tap, n_layers - 1);
        return false;
    }
    if (tap_bf16 && (tap < 0 || layers[tap].kind == XV_POOL)) {
        why = "the bf16 store can be tapped at a tdnn or affine layer only";
        return false;
    }
    if (n_seg < 0 || (n_seg > 0 && !lengths)) {
        why = "null argument (the segments' frame counts)";
        return false;
    }
    if (scratch_bytes < 1) {
        why = fmt("a scratch bound of %lld bytes; raise the option xvector_scratch_mib", scratch_bytes);
        return false;
    }
    p.last = tap < 0 ? n_layers - 1 : tap;
    p.n_seg = n_seg;
    const int S = n_layers + 1;
    for (int64_t i = 0; i < n_seg; i++) {
        if (lengths[i] < (int64_t)m.context + 1) {
            why = fmt("segment %lld holds %lld frames; the network needs %lld (its context of %lld frames + 1): pass longer segments", i,
                      lengths[i], (long long)m.context + 1, m.context);
            return false;
        }
        if (lengths[i] > (int64_t)1 << 30) {
            why = fmt("segment %lld holds %lld frames; at most 2^30: cut it into windows", i, lengths[i]);
            return false;
        }
        const int64_t need = xv_segment_bytes(m, lengths[i], p.last, tap_bf16);
        if (need > scratch_bytes) {
            why = fmt("segment %lld alone takes %lld bytes of activations, the bound is %lld; raise the option xvector_scratch_mib or cut the "
                      "segment into windows", i, need, scratch_bytes);
            return false;
        }
    }
    int64_t i = 0;
    while (i < n_seg) {
        XvChunk c;
        c.seg_begin = i;
        c.stage_rows.assign((size_t)S, 0);
        while (i < n_seg) {
            const int64_t need = xv_segment_bytes(m, lengths[i], p.last, tap_bf16);
            if (i > c.seg_begin && c.bytes + need > scratch_bytes) break;
            c.bytes += need;
            for (int s = 0; s < S; s++) c.stage_rows[(size_t)s] += xv_stage_rows(m, lengths[i], s);
            i++;
        }
        c.seg_end = i;
        const int top_stage = p.last >= m.pool ? m.pool : (tap_bf16 ? p.last + 1 : p.last);
        for (int s = 0; s <= top_stage; s++)
            p.buf_bytes[s & 1] = std::max(p.buf_bytes[s & 1], c.stage_rows[(size_t)s] * m.width_pad[(size_t)s] * 2);
        p.out_rows += c.stage_rows[(size_t)p.last + 1];
        p.chunks.push_back(std::move(c));
    }
    p.out_cols = m.width[(size_t)p.last + 1];
    return true;
}

void xv_layer_tiles(const XvModelInfo &m, const int64_t *lengths, int64_t seg_begin, int64_t seg_end, int l, std::vector<XvTile> &tiles) {
    tiles.clear();
    if (l > m.pool) {      // the pooled matrix: one run of rows, a row per segment
        const int64_t n = seg_end - seg_begin;
        for (int64_t f = 0; f < n; f += XV_TM) tiles.push_back({0, (int32_t)f, (int32_t)std::min<int64_t>(XV_TM, n - f), 0});
        return;
    }
    for (int64_t i = seg_begin; i < seg_end; i++) {
        const int64_t n = xv_stage_rows(m, lengths[i], l + 1);
        for (int64_t f = 0; f < n; f += XV_TM)
            tiles.push_back({(int32_t)(i - seg_begin), (int32_t)f, (int32_t)std::min<int64_t>(XV_TM, n - f), 0});
    }
}

bool xv_check_segments(const XvModelInfo &m, const int64_t *utt_offsets, int n_utt, const int32_t *segs, int64_t n_seg, std::string &why) {
    if (n_seg < 0 || (n_seg > 0 && !segs) || !utt_offsets) {
        why = "null argument (the segment table)";
        return false;
    }
    for (int64_t i = 0; i < n_seg; i++) {
        const int64_t u = segs[3 * i], first = segs[3 * i + 1], n = segs[3 * i + 2];
        if (u < 0 || u >= n_utt) {
            why = fmt("segment %lld names utterance %lld; the batch holds %lld", i, u, n_utt);
            return false;
        }
        const int64_t T = utt_offsets[u + 1] - utt_offsets[u];
        if (first < 0 || n < 0 || first + n > T) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "segment %lld covers frames %lld .. %lld of utterance %lld, which holds %lld; keep segments inside "
                          "their utterance", (long long)i, (long long)first, (long long)(first + n), (long long)u, (long long)T);
            why = buf;
            return false;
        }
        if (n < (int64_t)m.context + 1) {
            why = fmt("segment %lld holds %lld frames; the network needs %lld (its context of %lld frames + 1): pass longer segments", i, n,
                      (long long)m.context + 1, m.context);
            return false;
        }
    }
    return true;
}

}  // namespace sr
