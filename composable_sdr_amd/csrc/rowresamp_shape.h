// The launch shape of k_rowresamp (kernels_rowresamp.hip): taps per phase, outputs per tile, the LDS of a
// workgroup, and how a call of n_out outputs on nchan rows is cut into (row, tile) items and runs of consecutive items.  Pure
// functions of delta (Q32.32 input samples per output), m, the sample kind, the output count, the row count, the CU count and
// the carried time T; nothing here needs the HIP headers, so a host-only program can include it (csdr_rowresamp_launch_shape
// hands it to tests/test_rowresamp_cpu.py).  The kernel's index arithmetic uses the same functions.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RRS_HD __host__ __device__
#else
#define RRS_HD
#endif

namespace csdr {

constexpr uint32_t RRS_THREADS = 512;                // threads per workgroup
constexpr uint32_t RRS_NPFB = 256;                   // phases of the bank; it has RRS_NPFB + 1 rows
// The bank's image in LDS is [j][column(b)].  The lanes of a wave sit on consecutive outputs, whose phases advance by
// (delta >> 24) mod 256: at rates such as 8/5 or 4/5 that step is a multiple of 32, and in a plain [j][b] image the handful of
// phases a wave meets would all sit on one of the 32 banks a ds_read_b32 sees.  column(b) = b ^ (b >> 5) moves phases that are
// multiples of 32 apart onto different banks and keeps 32 consecutive phases on 32 different ones.  b <= 256, so a column is at
// most 256 ^ 8 = 264.  -DRRS_LINEAR_BANK builds the plain image, for A/B timings
#if defined(RRS_LINEAR_BANK)
constexpr uint32_t RRS_BANK_STRIDE = RRS_NPFB + 1;
RRS_HD constexpr uint32_t rrs_bank_col(uint32_t b) { return b; }
#else
constexpr uint32_t RRS_BANK_STRIDE = 265;            // floats from tap j to tap j + 1: odd, above the largest column
RRS_HD constexpr uint32_t rrs_bank_col(uint32_t b) { return b ^ (b >> 5); }
#endif
constexpr uint32_t RRS_MAX_SEMI = 8, RRS_MAX_SEMI_D = 56;
constexpr uint64_t RRS_MIN_DELTA = 1ull << 29, RRS_MAX_DELTA = 1ull << 35;   // r = 8 .. 1/8
constexpr uint32_t RRS_WINDOW_GOAL = 4096;           // slots a tile of 1024 outputs may span; a longer span gets 512 outputs
constexpr size_t RRS_LDS_LIMIT = 160 * 1024;         // a CU's LDS
constexpr uint32_t RRS_MAX_WGS_PER_CU = 4;           // 8 waves per workgroup: all 32 wave slots of a CU (the kernel needs <= 64 VGPRs for that)

// D = 1 for r >= 1, else ceil(1 / r), from the quantised rate 2^32 / delta: ceil(delta / 2^32)
RRS_HD constexpr uint32_t rrs_D(uint64_t delta) { return delta <= (1ull << 32) ? 1u : (uint32_t)((delta + 0xffffffffull) >> 32); }
RRS_HD constexpr uint32_t rrs_P(uint64_t delta, uint32_t m) { return 2 * m * rrs_D(delta); }
RRS_HD constexpr bool rrs_args_ok(uint64_t delta, uint32_t m)
{
    return delta >= RRS_MIN_DELTA && delta <= RRS_MAX_DELTA && m >= 1 && m <= RRS_MAX_SEMI && m * rrs_D(delta) <= RRS_MAX_SEMI_D;
}
// the time of output k of a call, relative to the call's first sample, and its sample, phase and fraction
RRS_HD constexpr uint64_t rrs_time(uint64_t T, uint64_t delta, uint32_t k) { return T + (uint64_t)k * delta; }
RRS_HD constexpr uint32_t rrs_sample(uint64_t t) { return (uint32_t)(t >> 32); }
RRS_HD constexpr uint32_t rrs_phase(uint64_t t) { return (uint32_t)(t >> 24) & 255u; }
RRS_HD constexpr uint32_t rrs_frac24(uint64_t t) { return (uint32_t)t & 0xffffffu; }
// outputs of a call of n samples (n <= 2^28) that starts at time T, and the time the next call starts at
RRS_HD constexpr uint32_t rrs_count(uint64_t T, uint64_t delta, uint32_t n)
{
    return (T >> 32) >= n ? 0u : (uint32_t)((((uint64_t)n << 32) - 1 - T) / delta) + 1;
}
RRS_HD constexpr uint64_t rrs_next_time(uint64_t T, uint64_t delta, uint32_t n, uint32_t n_out)
{
    return T + (uint64_t)n_out * delta - ((uint64_t)n << 32);
}
// window slots that `outs` consecutive outputs can span whatever their first one's fraction: the samples n_first - (P - 1) .. n_last
RRS_HD constexpr uint32_t rrs_span(uint64_t delta, uint32_t m, uint32_t outs)
{
    return (uint32_t)(((uint64_t)(outs - 1) * delta + 0xffffffffull) >> 32) + rrs_P(delta, m);
}
// outputs per tile: 1024 where their span stays within RRS_WINDOW_GOAL slots, else 512 (a span of at most 4200 slots)
RRS_HD constexpr uint32_t rrs_tile_outputs(uint64_t delta, uint32_t m) { return rrs_span(delta, m, 1024) <= RRS_WINDOW_GOAL ? 1024u : 512u; }
RRS_HD constexpr uint32_t rrs_window_slots(uint64_t delta, uint32_t m) { return rrs_span(delta, m, rrs_tile_outputs(delta, m)); }
// bytes of LDS per workgroup: the bank [P][RRS_BANK_STRIDE] float | the window, float2 or float
RRS_HD constexpr size_t rrs_lds_bytes(uint64_t delta, uint32_t m, bool cplx)
{
    return 4 * (size_t)RRS_BANK_STRIDE * rrs_P(delta, m) + (cplx ? 8 : 4) * (size_t)rrs_window_slots(delta, m);
}
// tile `tile` of a row: its outputs [o0, o0 + cnt) and the window's first sample (negative: in the row's history)
struct RrsTile { uint32_t o0, cnt; int64_t base; uint32_t span; };
RRS_HD inline RrsTile rrs_tile(uint64_t T, uint64_t delta, uint32_t m, uint32_t n_out, uint32_t tile)
{
    const uint32_t TO = rrs_tile_outputs(delta, m);
    RrsTile t;
    t.o0 = tile * TO;
    t.cnt = n_out - t.o0 < TO ? n_out - t.o0 : TO;
    t.base = (int64_t)rrs_sample(rrs_time(T, delta, t.o0)) - (int64_t)(rrs_P(delta, m) - 1);
    t.span = (uint32_t)((int64_t)rrs_sample(rrs_time(T, delta, t.o0 + t.cnt - 1)) - t.base) + 1;
    return t;
}

struct RrsShape {
    uint32_t D, P;              // decimation stretch and taps per phase
    uint32_t TO;                // outputs per tile
    uint32_t window;            // window slots
    uint32_t tiles;             // tiles per row, ceil(n_out / TO); the last one may be ragged
    uint32_t items;             // nchan tiles; item i is tile i % tiles of row i / tiles
    uint32_t items_per_run;     // consecutive items one workgroup walks
    uint32_t runs;              // workgroups of the launch
    uint32_t wgs_per_cu;        // what the LDS leaves room for
    size_t lds;                 // bytes per workgroup
    bool ok;                    // false: the item count does not fit 32 bits
};
// Up to cus * wgs_per_cu runs: a short call gets one item per workgroup, a long call one run per workgroup slot, so that the bank
// is staged once per slot.  T does not change the cut (a tile is a stretch of output indices); it moves the tiles' windows
inline RrsShape rrs_shape(uint64_t delta, uint32_t m, bool cplx, uint32_t n_out, uint32_t nchan, uint32_t cus, uint64_t T)
{
    (void)T;
    RrsShape s{};
    s.D = rrs_D(delta); s.P = rrs_P(delta, m);
    s.TO = rrs_tile_outputs(delta, m);
    s.window = rrs_window_slots(delta, m);
    s.lds = rrs_lds_bytes(delta, m, cplx);
    const size_t fit = RRS_LDS_LIMIT / s.lds;
    s.wgs_per_cu = (uint32_t)(fit < RRS_MAX_WGS_PER_CU ? fit : RRS_MAX_WGS_PER_CU);
    s.tiles = n_out / s.TO + (n_out % s.TO ? 1u : 0u);
    const uint64_t items = (uint64_t)s.tiles * nchan;
    s.ok = items <= 0xffffffffull;
    if (!s.ok) return s;
    s.items = (uint32_t)items;
    const uint32_t slots = (cus ? cus : 1u) * (s.wgs_per_cu ? s.wgs_per_cu : 1u);
    s.items_per_run = s.items ? (s.items - 1) / slots + 1 : 0;
    s.runs = s.items ? (s.items - 1) / s.items_per_run + 1 : 0;
    return s;
}

}  // namespace csdr
