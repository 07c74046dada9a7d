// The launch shape of k_pfb2 (kernels_pfb2.hip) and, at the end, of k_pfb2s (kernels_pfb2s.hip, 4.18): frames per
// tile, the LDS of a workgroup, and how a call of `frames` frames is cut into runs of consecutive tiles.  Pure functions of M, m,
// the frame count and the CU count; nothing here needs the HIP headers, so a host-only program can include it
// (csdr_pfbch2_launch_shape and csdr_pfbsyn2_launch_shape hand it to tests/test_pfbch2_cpu.py and tests/test_pfbsyn2_cpu.py).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PFB2_HD __host__ __device__
#else
#define PFB2_HD
#endif

namespace csdr {

constexpr uint32_t PFB2_THREADS = 512;               // threads per workgroup
constexpr uint32_t PFB2_MIN_M = 4, PFB2_MAX_M = 256, PFB2_MAX_SEMI = 8;
constexpr size_t PFB2_LDS_LIMIT = 160 * 1024;        // a CU's LDS
constexpr uint32_t PFB2_MAX_WGS_PER_CU = 2;          // 8 waves per workgroup; the kernel asks for 4 waves per SIMD (128 VGPRs)

PFB2_HD constexpr bool pfb2_args_ok(uint32_t M, uint32_t m)
{
    return M >= PFB2_MIN_M && M <= PFB2_MAX_M && (M & (M - 1)) == 0 && m >= 1 && m <= PFB2_MAX_SEMI;
}
// frames per tile: 4096 / M, a tile of 4096 (frame, branch) items, and never fewer than 16 (a row piece of 128 bytes)
PFB2_HD constexpr uint32_t pfb2_tile_frames(uint32_t M) { return 4096u / M; }
// float2 slots of the sample window: the L - M/2 samples in front of a tile and its F M/2 new ones
PFB2_HD constexpr uint32_t pfb2_window_slots(uint32_t M, uint32_t m) { return 2 * m * M - M / 2 + pfb2_tile_frames(M) * (M / 2); }
// float2 slots from one frame of V to the next.  The DFT and the store pass put a half-wave's lanes on consecutive frames: an odd stride
// spreads 32 frames over the 64 banks; at 16 frames per tile the stride is twice an odd number and the half-wave's other 16 lanes work
// an odd number of slots away
PFB2_HD constexpr uint32_t pfb2_row_stride(uint32_t M) { return pfb2_tile_frames(M) >= 32 ? M + 1 : M + 2; }
// bytes of LDS per workgroup: window | V [F][row stride] | twiddles [M / 4], all float2
PFB2_HD inline size_t pfb2_lds_bytes(uint32_t M, uint32_t m)
{
    const size_t F = pfb2_tile_frames(M);
    return 8 * ((size_t)pfb2_window_slots(M, m) + F * pfb2_row_stride(M) + M / 4);
}

struct Pfb2Shape {
    uint32_t F;                 // frames per tile
    uint32_t tiles;             // ceil(frames / F); the last one may be ragged
    uint32_t tiles_per_run;     // consecutive tiles one workgroup walks
    uint32_t runs;              // workgroups of the launch
    uint32_t wgs_per_cu;        // what the LDS leaves room for
    size_t lds;                 // bytes per workgroup
};
// Up to cus * wgs_per_cu runs: a short call gets one tile per workgroup and so as many CUs as it has tiles, a long call gets one
// run per workgroup slot, so that the L - M/2 halo samples are read once per slot
inline Pfb2Shape pfb2_shape(uint32_t M, uint32_t m, uint32_t frames, uint32_t cus)
{
    Pfb2Shape s{};
    s.F = pfb2_tile_frames(M);
    s.lds = pfb2_lds_bytes(M, m);
    const size_t fit = PFB2_LDS_LIMIT / s.lds;
    s.wgs_per_cu = (uint32_t)(fit < PFB2_MAX_WGS_PER_CU ? fit : PFB2_MAX_WGS_PER_CU);
    s.tiles = (frames + s.F - 1) / s.F;
    const uint32_t slots = (cus ? cus : 1u) * (s.wgs_per_cu ? s.wgs_per_cu : 1u);
    s.tiles_per_run = s.tiles ? (s.tiles + slots - 1) / slots : 0;
    s.runs = s.tiles ? (s.tiles + s.tiles_per_run - 1) / s.tiles_per_run : 0;
    return s;
}

// ---- k_pfb2s, the synthesizer (kernels_pfb2s.hip): the same tiles, runs and row stride; only the LDS differs ----
// float2 slots of the accumulator carry: the L - M/2 partial sums behind a tile.  The tile's own F M/2 sums are final when its FIR
// ends and leave from registers, so they have no slot
PFB2_HD constexpr uint32_t pfb2s_carry_slots(uint32_t M, uint32_t m) { return 2 * m * M - M / 2; }
// frames in front of a run that reach into it (and that the handle carries from call to call): 4 m - 1
PFB2_HD constexpr uint32_t pfb2s_halo_frames(uint32_t m) { return 4 * m - 1; }
// bytes of LDS per workgroup: carry | V [F][row stride] | twiddles [M / 4], all float2, | the 2 m M taps, float
PFB2_HD inline size_t pfb2s_lds_bytes(uint32_t M, uint32_t m)
{
    const size_t F = pfb2_tile_frames(M);
    return 8 * ((size_t)pfb2s_carry_slots(M, m) + F * pfb2_row_stride(M) + M / 4) + 4 * (size_t)(2 * m * M);
}
// pfb2_shape's cut of a call into runs of tiles with the synthesizer's LDS.  A run's tiles are counted in output frames; the
// kernel walks ceil((its frames + 4 m - 1) / F) tiles of input frames, the halo in front included
inline Pfb2Shape pfb2s_shape(uint32_t M, uint32_t m, uint32_t frames, uint32_t cus)
{
    Pfb2Shape s{};
    s.F = pfb2_tile_frames(M);
    s.lds = pfb2s_lds_bytes(M, m);
    const size_t fit = PFB2_LDS_LIMIT / s.lds;
    s.wgs_per_cu = (uint32_t)(fit < PFB2_MAX_WGS_PER_CU ? fit : PFB2_MAX_WGS_PER_CU);
    s.tiles = (frames + s.F - 1) / s.F;
    const uint32_t slots = (cus ? cus : 1u) * (s.wgs_per_cu ? s.wgs_per_cu : 1u);
    s.tiles_per_run = s.tiles ? (s.tiles + slots - 1) / slots : 0;
    s.runs = s.tiles ? (s.tiles + s.tiles_per_run - 1) / s.tiles_per_run : 0;
    return s;
}

}  // namespace csdr
