// xvector_checks.cpp -- csrc/xvector_plan.cpp (what the x-vector forward pass decides before it touches the device) under the host
// sanitizers: a stand-alone program, built by tests/test_xvector_cpu.py with g++ -fsanitize=address,undefined.  It sweeps the plan
// over networks, ragged segment lists, taps and scratch bounds and walks every tile list the way the layer kernel does: every row a
// tile reads or writes must lie inside its own segment's rows of the stage, the tiles of a layer must cover every output row once,
// and the chunk's buffers must hold every stage.
#include "xvector_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sr;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                             \
        }                                                                           \
    } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

static XvLayer tdnn(int c_in, int c_out, std::vector<int> off, int act = XV_ACT_RELU) {
    XvLayer L;
    L.kind = XV_TDNN;
    L.c_in = c_in;
    L.c_out = c_out;
    L.act = act;
    L.n_off = (int)off.size();
    for (size_t j = 0; j < off.size() && j < (size_t)XV_MAX_OFFSETS; j++) L.off[j] = off[j];
    return L;
}

static XvLayer pool(int c) {
    XvLayer L;
    L.kind = XV_POOL;
    L.c_in = c;
    L.c_out = 2 * c;
    L.var_floor = 1e-10;
    return L;
}

static XvLayer affine(int c_in, int c_out, int act = XV_ACT_NONE) {
    XvLayer L = tdnn(c_in, c_out, {0}, act);
    L.kind = XV_AFFINE;
    return L;
}

static void walk(const std::vector<XvLayer> &net, const std::vector<int64_t> &len, int tap, bool tap_bf16, int64_t bound) {
    XvPlan p;
    std::string why;
    const bool ok = plan_xvector(net.data(), (int)net.size(), len.data(), (int64_t)len.size(), tap, tap_bf16, bound, p, why);
    if (!ok) {
        CHECK(!why.empty());
        return;
    }
    const XvModelInfo &m = p.info;
    const int L = m.n_layers;
    CHECK(p.last == (tap < 0 ? L - 1 : tap));
    int64_t next = 0, out_rows = 0;
    for (const XvChunk &c : p.chunks) {
        CHECK(c.seg_begin == next && c.seg_end > c.seg_begin);
        next = c.seg_end;
        int64_t bytes = 0;
        for (int64_t i = c.seg_begin; i < c.seg_end; i++) bytes += xv_segment_bytes(m, len[(size_t)i], p.last, tap_bf16);
        CHECK(bytes == c.bytes);
        CHECK(c.bytes <= bound || c.seg_end - c.seg_begin == 1);
        const int top = p.last >= m.pool ? m.pool : (tap_bf16 ? p.last + 1 : p.last);
        int64_t need[2] = {0, 0};
        for (int s = 0; s <= top; s++) {
            const int64_t b = c.stage_rows[(size_t)s] * m.width_pad[(size_t)s] * 2;
            CHECK(b <= p.buf_bytes[s & 1]);
            need[s & 1] = std::max(need[s & 1], b);
        }
        CHECK(need[0] + need[1] <= c.bytes);      // the two ping-ponged buffers of this chunk are within what the chunk was charged
        out_rows += c.stage_rows[(size_t)p.last + 1];
        std::vector<XvTile> tiles;
        for (int l = 0; l <= p.last; l++) {
            if (l == m.pool) continue;
            xv_layer_tiles(m, len.data(), c.seg_begin, c.seg_end, l, tiles);
            const int64_t n = c.seg_end - c.seg_begin;
            std::vector<int64_t> covered((size_t)(l > m.pool ? 1 : n), 0);
            for (const XvTile &t : tiles) {
                CHECK(t.rows >= 1 && t.rows <= XV_TM && t.first >= 0 && t.first % XV_TM == 0);
                CHECK(t.seg >= 0 && t.seg < (int64_t)covered.size());
                if (t.seg < 0 || t.seg >= (int64_t)covered.size()) continue;
                const int64_t seg_rows_out = l > m.pool ? n : xv_stage_rows(m, len[(size_t)(c.seg_begin + t.seg)], l + 1);
                const int64_t seg_rows_in = l > m.pool ? n : xv_stage_rows(m, len[(size_t)(c.seg_begin + t.seg)], l);
                CHECK(t.first + t.rows <= seg_rows_out);                                       // no tile straddles a segment
                CHECK(t.first + t.rows - 1 + m.span[(size_t)l] <= seg_rows_in - 1);            // the last row read, at the last offset
                CHECK(t.first == covered[(size_t)t.seg]);                                      // in order, no gap, no overlap
                covered[(size_t)t.seg] += t.rows;
            }
            for (size_t i = 0; i < covered.size(); i++)
                CHECK(covered[i] == (l > m.pool ? n : xv_stage_rows(m, len[(size_t)c.seg_begin + i], l + 1)));
        }
    }
    CHECK(next == (int64_t)len.size() && out_rows == p.out_rows && p.out_cols == m.width[(size_t)p.last + 1]);
}

int main() {
    // ---- the model's refusals ----
    XvModelInfo info;
    std::string why;
    const std::vector<XvLayer> good = {tdnn(30, 512, {-2, -1, 0, 1, 2}), tdnn(512, 512, {-2, 0, 2}), tdnn(512, 512, {-3, 0, 3}), tdnn(512, 512, {0}),
                                       tdnn(512, 1500, {0}), pool(1500), affine(3000, 512)};
    CHECK(xv_check_model(good.data(), (int)good.size(), info, why));
    CHECK(info.context == 14 && info.pool == 5 && info.embedding_dim == 512 && info.input_dim == 30);
    CHECK(info.width_pad[0] == 32 && info.width_pad[5] == 1504 && info.width_pad[6] == 3008 && info.k_pad[0] == 192 && info.n_pad[4] == 1536);
    auto refused = [&](std::vector<XvLayer> net, const char *what) {
        XvModelInfo i2;
        std::string w;
        const bool ok = xv_check_model(net.data(), (int)net.size(), i2, w);
        if (ok || !has(w, what)) std::fprintf(stderr, "  (got: %s)\n", w.c_str());
        return !ok && has(w, what);
    };
    CHECK(refused({tdnn(30, 64, {0}), affine(64, 8)}, "exactly one"));
    CHECK(refused({tdnn(30, 64, {0}), pool(64), pool(128), affine(256, 8)}, "exactly one"));
    CHECK(refused({tdnn(30, 64, {0}), pool(64)}, "at least one affine layer follows"));
    CHECK(refused({tdnn(30, 64, {0}), pool(64), affine(128, 8, XV_ACT_RELU)}, "last layer's act must be none"));
    CHECK(refused({tdnn(30, 64, {0, -1}), pool(64), affine(128, 8)}, "ascend strictly"));
    CHECK(refused({tdnn(30, 64, {0, 0}), pool(64), affine(128, 8)}, "ascend strictly"));
    CHECK(refused({tdnn(30, 64, {-17}), pool(64), affine(128, 8)}, "within -16 .. 16"));
    CHECK(refused({tdnn(30, 64, {}), pool(64), affine(128, 8)}, "offsets; 1 .. 9"));
    CHECK(refused({tdnn(0, 64, {0}), pool(64), affine(128, 8)}, "input channels; 1 .. 4096"));
    CHECK(refused({tdnn(30, 4097, {0}), pool(4097), affine(8194, 8)}, "output channels; 1 .. 4096"));
    CHECK(refused({tdnn(30, 64, {0}), pool(65), affine(130, 8)}, "consecutive layers must agree"));
    CHECK(refused({tdnn(30, 64, {0}), pool(64), affine(127, 8)}, "consecutive layers must agree"));
    CHECK(refused({affine(30, 64), pool(64), affine(128, 8)}, "frame layers are tdnn"));
    CHECK(refused({tdnn(30, 64, {0}), pool(64), tdnn(128, 8, {0}, XV_ACT_NONE)}, "segment layers are affine"));

    // ---- the plan, walked ----
    const std::vector<XvLayer> small = {tdnn(24, 33, {-1, 0, 2}), tdnn(33, 200, {0, 4}), tdnn(200, 31, {-5}, XV_ACT_NONE), pool(31), affine(62, 17)};
    const std::vector<XvLayer> no_frame = {pool(33), affine(66, 5)};
    const std::vector<std::vector<int64_t>> lists = {{}, {15}, {15, 200, 457}, {8, 135, 136, 137, 8 + 2 * 128 + 3}, std::vector<int64_t>(70, 300),
                                                     {1000, 15, 15, 15, 999}};
    for (const auto &net : {good, small, no_frame})
        for (const auto &len : lists)
            for (int tap = -1; tap < (int)net.size(); tap++)
                for (int b16 = 0; b16 < 2; b16++)
                    for (int64_t bound : {(int64_t)1 << 20, (int64_t)5 << 20, XV_DEFAULT_SCRATCH, (int64_t)1, (int64_t)0}) walk(net, len, tap, b16 != 0, bound);

    // ---- the plan's refusals ----
    XvPlan p;
    const int64_t short_len[2] = {15, 14};
    CHECK(!plan_xvector(good.data(), 7, short_len, 2, -1, false, XV_DEFAULT_SCRATCH, p, why) && has(why, "segment 1 holds 14 frames; the network needs 15"));
    const int64_t long_len[1] = {100000};
    CHECK(!plan_xvector(good.data(), 7, long_len, 1, -1, false, (int64_t)1 << 20, p, why) && has(why, "segment 0 alone takes") &&
          has(why, "raise the option xvector_scratch_mib"));
    CHECK(!plan_xvector(good.data(), 7, short_len, 1, 7, false, XV_DEFAULT_SCRATCH, p, why) && has(why, "tap 7"));
    CHECK(!plan_xvector(good.data(), 7, short_len, 1, 5, true, XV_DEFAULT_SCRATCH, p, why) && has(why, "tdnn or affine layer only"));
    CHECK(!plan_xvector(good.data(), 7, nullptr, 1, -1, false, XV_DEFAULT_SCRATCH, p, why) && has(why, "null argument"));
    // chunking under 1 MiB: 70 segments of 300 frames of the standard network do not fit one chunk, every chunk is whole segments
    const std::vector<int64_t> many(70, 300);
    CHECK(plan_xvector(good.data(), 7, many.data(), 70, -1, false, (int64_t)2 << 20, p, why) && p.chunks.size() > 1);

    // ---- the segment table ----
    const int64_t off[3] = {0, 100, 140};
    const int32_t ok_segs[6] = {0, 0, 100, 1, 25, 15};
    CHECK(xv_check_segments(info, off, 2, ok_segs, 2, why));
    const int32_t past[3] = {1, 30, 15};
    CHECK(!xv_check_segments(info, off, 2, past, 1, why) && has(why, "segment 0 covers frames 30 .. 45 of utterance 1, which holds 40"));
    const int32_t no_utt[3] = {2, 0, 15};
    CHECK(!xv_check_segments(info, off, 2, no_utt, 1, why) && has(why, "names utterance 2"));
    const int32_t brief[3] = {0, 5, 14};
    CHECK(!xv_check_segments(info, off, 2, brief, 1, why) && has(why, "holds 14 frames; the network needs 15"));
    const int32_t neg[3] = {0, -1, 20};
    CHECK(!xv_check_segments(info, off, 2, neg, 1, why) && has(why, "keep segments inside"));

    // ---- the descriptor row ----
    const int32_t d[XV_DESC] = {XV_TDNN, 30, 512, XV_ACT_RELU, 1, 3, -3, 0, 3, 0, 0, 0, 0, 0, 0, 0};
    const XvLayer L = xv_layer_from_desc(d, 0.5);
    CHECK(L.kind == XV_TDNN && L.c_in == 30 && L.c_out == 512 && L.act == XV_ACT_RELU && L.has_affine && L.n_off == 3 && L.off[0] == -3 && L.off[2] == 3);

    if (failures) {
        std::fprintf(stderr, "%d xvector checks failed\n", failures);
        return 1;
    }
    std::printf("xvector checks ok\n");
    return 0;
}
