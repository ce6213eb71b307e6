// The ConvNeXt layer stream's plan (fv_cnxstream_*, engine_cnxstream.hip): which frames every level computes in one call, and where they
// lie.  Host arithmetic only — this header compiles without HIP, so a frame-by-frame simulation can run it on the CPU.
//
// p = 3 (a k = 7 'same' conv).  Level 0 is the stem conv, levels 1 .. L the blocks.  After N frames have arrived, level l's output is known
// on [0, front(N, l)): front = N at a flush (the zero padding past N is then the true one), else max(0, N - p (l + 1)).  Level L's frontier
// is the emission frontier: R = p (L + 1).
//
// Level l >= 1 reads level l - 1's output: the frames below that level's OLD frontier from the block's ring (slot = frame & (cap - 1)), the
// frames [in0, in1) — what level l - 1 produced in this call — from the linear chunk.  Output column t needs the frames t - 3 .. t + 3:
// at least in0 - 6 (out0 >= in0 - 3), so the ring keeps 6 frames below a frontier and takes one call's frames on top, cap >= 6 + step with
// step = max(max_chunk, R) (a flush moves a frontier by up to R).  The launch that reads the ring files the chunk into it: the frames read,
// [in0 - 6, in0), and the frames written, [in0, in1), span at most cap slots, so no slot is read in the launch that writes it.
#pragma once

namespace fv {

constexpr int kCnxPad = 3;          // (7 - 1) / 2
constexpr int kCnxHalo = 2 * kCnxPad;
constexpr int kCnxTile = 32;        // output columns per workgroup of the depthwise kernel (DWT_TT)

inline long long cnx_front(long long N, int level, bool flush) {
    const long long f = N - (long long)kCnxPad * (level + 1);
    return flush ? N : (f > 0 ? f : 0);
}
inline int cnx_reach(int levels_above_stem) { return kCnxPad * (levels_above_stem + 1); }
// the most frames one call adds to a frontier
inline int cnx_step(int max_chunk, int L) { return max_chunk > cnx_reach(L) ? max_chunk : cnx_reach(L); }
// The session pool (fv_cnxpool_*): an item may carry frames AND flush in one step, so a frontier moves by up to max_chunk + R frames
inline int cnx_pool_step(int max_chunk, int L) { return max_chunk + cnx_reach(L); }
inline int cnx_ring_cap(int step) {
    int cap = 1;
    while (cap < kCnxHalo + step) cap <<= 1;
    return cap;
}

// The stem: conv_layer_run over the window [N0 - 6, N1) (frames < 0 are zeros), W = 6 + c columns; its output columns [out0, out1) are
// kept, column `off` of the window onward.  The window kernel reads the input ring's [N0 - 6, N0) and files [N0, N1).
struct CnxStemPlan {
    long long out0, out1;
    int W, off;
};
inline CnxStemPlan cnx_stem_plan(long long N0, long long N1, bool flush) {
    CnxStemPlan s;
    s.out0 = cnx_front(N0, 0, false), s.out1 = cnx_front(N1, 0, flush);
    s.W = (int)(N1 - N0) + kCnxHalo;
    s.off = (int)(s.out0 - (N0 - kCnxHalo));
    return s;
}

// A block, level l >= 1.  Workgroup j of a row owns the output columns [out0 + 32 j, + 32) and stages the frames 3 below to 3 above them;
// it files the staged frames of [in0, in1) from its column 3 on (workgroup 0: from in0 on), so every chunk frame is filed exactly once.
// A level with no output columns yet still files its chunk: tiles covers the chunk as well as the outputs.
struct CnxLevelPlan {
    long long in0, in1;      // the chunk: level l - 1's new frames; the ring serves [in0 - 6, in0)
    long long out0, out1;    // the new output columns
    int tiles;               // workgroups per row; 0: nothing to launch
};
inline CnxLevelPlan cnx_level_plan(long long N0, long long N1, bool flush, int level) {
    CnxLevelPlan q;
    q.in0 = cnx_front(N0, level - 1, false), q.in1 = cnx_front(N1, level - 1, flush);
    q.out0 = cnx_front(N0, level, false), q.out1 = cnx_front(N1, level, flush);
    long long span = q.out1 - q.out0;
    if (q.in1 - kCnxPad - q.out0 > span) span = q.in1 - kCnxPad - q.out0;
    if (q.in1 > q.in0 && span < 1) span = 1;
    q.tiles = span > 0 ? (int)((span + kCnxTile - 1) / kCnxTile) : 0;
    return q;
}
// first frame workgroup j files (it files up to its window's end, out0 + 32 j + 35, and never past in1)
inline long long cnx_file_from(const CnxLevelPlan& q, int j) { return j == 0 ? q.in0 : q.out0 + (long long)kCnxTile * j + kCnxPad; }

}  // namespace fv
