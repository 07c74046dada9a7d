// The launch shape of the time-parallel AGC tail (kernels_agc_tail.hip): its knobs, which calls take the tile-major kernel, how a call
// of nf frames is cut into segments and what grids that gives, and how the segment tables are sized.  Pure functions of the knobs the
// tail read when it was made, the channel count and nf.  Included by the tail through csdr_internal.h and, on its own, by host-only
// programs (tests/test_agc_tail_shape.py): nothing here needs the HIP headers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace csdr {

constexpr uint32_t TM_CK = 256;         // samples between the checkpoints of a segment
constexpr uint32_t TM_GUARD = 512;      // blocks of 16 samples: >= max(W, L) / 16 of the tile-major route (W, L <= TM_MAX)
constexpr uint32_t TM_MAX = 8192;       // the warm-up and the segments of the tile-major route stay inside the guards: TM_GUARD x 16
constexpr uint32_t TM_L_RULE_MAX = TM_MAX - 32u;    // the longest segment the tile-major rule chooses (whole 32-sample block pairs)
constexpr uint32_t TM_L_KNOB_MAX = TM_MAX - 16u;    // the longest CSDR_AGC_L_TM (whole 16-sample blocks; the block-pair rounding makes it TM_MAX)

// The knobs of one tail, fixed when it is made
struct AgcTailKnobs {
    uint32_t L = 0;                 // row-major route: fixed segment length (CSDR_AGC_L), 0 = chosen per call
    uint32_t L_tm = 0;              // tile-major route: fixed segment length (CSDR_AGC_L_TM), 0 = chosen per call
    uint32_t W = 1024;              // warm-up samples in front of a segment (CSDR_AGC_W)
    uint32_t Lmin = 384;
    uint32_t wg_slots = 1024;       // workgroups the device holds at once
    bool tm_off = false;            // CSDR_AGC_TM=0 (A/B): the row-major route for every call
    // from the texts of the variables (null: not set) and the CU count of the handle's device
    static AgcTailKnobs parse(uint32_t cus, const char *l, const char *l_tm, const char *w, const char *wgs, const char *cus_knob, const char *tm)
    {
        AgcTailKnobs k;
        if (l) { k.L = (uint32_t)atol(l); k.L = (k.L + 15u) / 16u * 16u; if (k.L < 16) k.L = 16; }
        if (l_tm) { k.L_tm = ((uint32_t)atol(l_tm) + 15u) / 16u * 16u; if (k.L_tm < 16) k.L_tm = 16; if (k.L_tm > TM_L_KNOB_MAX) k.L_tm = TM_L_KNOB_MAX; }
        if (w) k.W = (uint32_t)atol(w);
        k.W = (k.W + 15u) / 16u * 16u;
        if (cus_knob && atoi(cus_knob) > 0 && (uint32_t)atoi(cus_knob) < cus) cus = (uint32_t)atoi(cus_knob);      // experiments: a plan sized for a CU-masked stream
        // k_agc_spec: two waves per workgroup at <= 256 VGPRs -> two waves per SIMD -> four workgroups per CU
        k.wg_slots = cus * 4u;
        if (wgs) k.wg_slots = cus * (uint32_t)(atol(wgs) > 0 ? atol(wgs) : 1);
        k.tm_off = tm && atoi(tm) == 0;
        return k;
    }
};

// the tile-major kernel packs 64 rows into a workgroup: a channel count that is a multiple or a divisor of 64
inline bool agc_tail_tm_channels_ok(uint32_t C) { return C % 64u == 0 || (C < 64u && 64u % C == 0); }

// the tile-major route (k_agc_spec_tm): whole 16-frame blocks, at least two segments, channel count a multiple or a divisor of 64
inline bool agc_tail_tm_supported(const AgcTailKnobs &k, uint32_t C, uint32_t nf)
{
    if (k.tm_off || !nf || nf % 16u || k.W > TM_MAX || k.W % 16u) return false;
    if (!agc_tail_tm_channels_ok(C)) return false;
    if (nf < 4u * k.W) return false;                             // short calls: a handful of segments, the row-major kernel's ground
    if (((uint64_t)nf / 16u + 2ull * TM_GUARD) * C * 128ull >= (1ull << 32)) return false;        // 32-bit byte offsets inside the plane
    return true;
}
inline size_t agc_tail_tm_guard(uint32_t C) { return (size_t)TM_GUARD * 16u * C; }       // float2 elements in front of and behind a tile-major plane

// the tables of a tail for calls of up to max_nf frames: segment records per channel, checkpoint records in all
struct AgcTailSizes { uint32_t max_seg; size_t ckpt_cap; };
inline AgcTailSizes agc_tail_sizes(uint32_t C, uint32_t max_nf)
{
    return {(max_nf + 15u) / 16u + 1,                            // L >= 16
            (size_t)C * ((size_t)max_nf / 128u + 64u)};          // >= nseg x ceil(L / TM_CK) for every L >= 128 of the tile-major route
}

struct AgcTailShape {
    uint32_t L, nseg, nck;          // segment length, segments and checkpoints per segment of a row
    bool pairs;                     // row-major kernel: 16-byte pieces
    uint32_t ls, groups, grid;      // row-major kernel: 2^ls segments x 64 >> ls channels per workgroup, segment groups per row, workgroups
    uint32_t Cw, nsub, ncg, grid_tm;// tile-major kernel: channels per workgroup, segments per workgroup, channel groups, workgroups
};

// One call of nf >= 1 frames on C >= 1 channels; tm: a call agc_tail_tm_supported() accepts, as a tile-major plane.
// Segment length: as many 64-segment groups per channel as the device holds workgroups at once (one round, every
// SIMD busy), not more -- shorter segments re-read more warm-up ((W + L) / L times the data) and a second round of
// workgroups costs more than it brings.  L / 16 is made odd: with a power-of-two L the 64 streams of a group and
// the groups of all channels hit the same few HBM channels at every step (L = 1024: 0.37 ms, 1040: 0.34 ms).
inline AgcTailShape agc_tail_shape(const AgcTailKnobs &k, uint32_t C, uint32_t nf, bool tm)
{
    AgcTailShape h{};
    h.Cw = C < 64u ? C : 64u; h.nsub = 64u / h.Cw; h.ncg = C / h.Cw;
    uint32_t L = tm ? k.L_tm : k.L;
    // tile-major route: the two-thirds rule below gives L >= 384 on its own once the plane passes ~128 MiB; below that the device is
    // under-filled and the re-reads come out of the L2s / the MALL, so shorter segments pay (round 5, profiles/r05_call_size_sweeps.txt:
    // 256 channels x 16 384 frames 153 -> 137 us, 1024 x 4096 151 -> 136 us with 128 against 384; nothing below 128)
    const uint32_t lmin_tm = 128u;
    if (!L && tm) {
        // two thirds of the workgroups the device holds at once (ncg channel groups x nseg / nsub segment groups): measured optimum
        // between the warm-up re-reads ((W + L) / L times the plane, shorter segments) and the blocks a workgroup walks (longer ones);
        // profiles/r04_agc_tm_segment_sweep.txt
        uint64_t nseg_t = (uint64_t)k.wg_slots * h.nsub * 2u / (3u * h.ncg);
        if (nseg_t < 2) nseg_t = 2;
        L = (uint32_t)((nf + nseg_t - 1) / nseg_t);
        L = (L + 31u) / 32u * 32u;                               // F32 rows leave as whole 128-byte lines per block pair
        if (L < lmin_tm) L = lmin_tm;
        if (L > TM_L_RULE_MAX) L = TM_L_RULE_MAX;
    }
    if (tm && L < lmin_tm) L = lmin_tm;                          // (CSDR_AGC_L_TM below the plan's bounds: the checkpoint table is sized for L >= lmin_tm)
    if (tm && (L % 32u)) L = (L + 31u) / 32u * 32u;
    if (!L) {
        // as many segments per row as the device has lanes for (the kernel packs the segments of several channels into a workgroup when
        // a row has few)
        const uint64_t nseg_t = 64ull * k.wg_slots / C ? 64ull * k.wg_slots / C : 1ull;
        L = (uint32_t)((nf + nseg_t - 1) / nseg_t);
        L = (L + 15u) / 16u * 16u;
        // Lmin bounds the warm-up re-reads ((W + L) / L times the plane) of a bandwidth-bound call.  A call whose whole plane sits in the
        // L2s (the reference's own 4096-frame chunk: 8 MiB at 256 channels) is bound by the walk instead -- (W + L) samples of a ~200-cycle
        // recurrence per lane -- and 11 segments of 400 left 53 of a workgroup's 64 lanes idle: such calls take every segment the device
        // has a lane for (round 5: 161 -> ~120 us per reference chunk)
        const uint32_t lmin = ((uint64_t)C * nf * 8u <= (24ull << 20)) ? 16u : k.Lmin;     // (8: bytes per CF32 sample)
        if (L < lmin) L = lmin;
        if (((L / 16u) & 1u) == 0) L += 16u;
    }
    h.L = L;
    h.nseg = (nf + L - 1) / L;
    h.nck = (L + TM_CK - 1u) / TM_CK;
    // PAIRS: nf even, so every row starts on a 16-byte boundary and ends on one (t is always even): a piece is one
    // 16-byte load that never reaches past the buffer
    h.pairs = (nf & 1u) == 0 && (uint64_t)C * nf >= 2;
    // row-major kernel: spw segments x cpw channels per workgroup (cpw > 1 needs whole-piece rows and 32-bit offsets inside its rows)
    h.ls = 6;
    if (h.nseg <= 32u && h.pairs && (nf & 3u) == 0 && C >= 8u && (uint64_t)nf * 64ull < (1ull << 32)) { h.ls = 3; while ((1u << h.ls) < h.nseg) h.ls++; }
    const uint32_t spw = 1u << h.ls, cpw = 64u >> h.ls;
    h.groups = (h.nseg + spw - 1u) / spw;
    h.grid = ((C + cpw - 1u) / cpw) * h.groups;
    h.grid_tm = h.ncg * ((h.nseg + h.nsub - 1) / h.nsub);
    return h;
}

}  // namespace csdr
