// What k_psktrack (kernels_psktrack.hip) and the host share: the launch shape, the layout of a row's state record,
// and the two functions of the "csdr psktrack v1" contract that the host exposes or restates: sine and cosine of a phase word and
// word(), radians -> phase words.  Both are plain f32 in a fixed order with no contraction; tests/psktrack_restatement.py
// restates them bit for bit.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSK_HD __host__ __device__ __forceinline__
#else
#define PSK_HD inline
#endif

namespace csdr {

constexpr uint32_t PSK_SL = 64;          // rows per workgroup: one wave, one lane each
constexpr uint32_t PSK_SB = 16;          // input samples per LDS block
constexpr uint32_t PSK_XS = PSK_SB + 1;  // a row's slot in the staged block, in pairs: odd, so the lanes of a half wave meet different bank pairs
constexpr uint32_t PSK_MAX_EQ = 17;      // equaliser taps
// a row's state record in HBM, in 32-bit words: live (0: the state right after new), p, theta, freq, parity, symbol count, two
// spare words; then the weights w[L] and the window buf[L] (oldest sample first) as (re, im) pairs
constexpr uint32_t PSK_HDR = 8;
constexpr uint32_t psk_state_words(uint32_t L) { return PSK_HDR + 4 * L; }
// a lane's weights and window in LDS, in pairs: w[L] | buf[L], padded to an odd stride
constexpr uint32_t psk_win_stride(uint32_t L) { return L ? ((2 * L) | 1u) : 0u; }
constexpr size_t psk_lds_bytes(uint32_t L) { return 8 * (size_t)PSK_SL * (PSK_XS + psk_win_stride(L)); }

constexpr float PSK_P_MIN = 7.8886090522101181e-31f;      // 2^-100: the floor of the power estimate
constexpr float PSK_EQ_EPS = 9.5367431640625e-07f;        // 2^-20: eps of the normalised LMS
constexpr float PSK_A_QPSK = 0.70710677f;                 // the QPSK points are (+-A +-jA)

// (sin, cos) of the phase word w, 2^32 = one turn.  Octant o = w >> 29; remainder r = w & (2^29 - 1), reflected to 2^29 - r in the
// odd octants, so a = f32(r) * f32(pi 2^-31) lies in [0, pi / 4].  z = a a;
//   sin a = ((((S3 z + S2) z + S1) z) a) + a        cos a = (1 - 0.5 z) + ((((C3 z + C2) z + C1) z) z)
// every operation rounded once (the coefficients are the single-precision minimax sets of the Cephes library).  Octants 1, 2, 5, 6
// swap the two, sin is negated in octants 4 .. 7, cos in octants 2 .. 5.
PSK_HD void psk_sincos_word(uint32_t w, float *sn, float *cs)
{
#pragma clang fp contract(off)
    const uint32_t o = w >> 29;
    int32_t r = (int32_t)(w & 0x1fffffffu);
    if (o & 1u) r = 0x20000000 - r;
    const float a = (float)r * 1.4629180792671596e-09f;   // pi 2^-31
    const float z = a * a;
    float p = -1.9515295891e-4f * z;
    p = p + 8.3321608736e-3f;
    p = p * z;
    p = p + -1.6666654611e-1f;
    p = p * z;
    p = p * a;
    const float s = p + a;
    float q = 2.443315711809948e-5f * z;
    q = q + -1.388731625493765e-3f;
    q = q * z;
    q = q + 4.166664568298827e-2f;
    q = q * z;
    q = q * z;
    const float h = 0.5f * z;
    const float u = 1.0f - h;
    const float c = u + q;
    const bool swap = ((o + 1u) >> 1) & 1u;
    float ys = swap ? c : s, yc = swap ? s : c;
    if (o >= 4u) ys = -ys;
    if (((o + 2u) >> 2) & 1u) yc = -yc;
    *sn = ys;
    *cs = yc;
}

// radians -> phase words: one f32 product by 2^31 / pi, NaN -> 0, clamped to +-2^30, rounded to the nearest integer (ties to
// even); the caller adds it modulo 2^32
PSK_HD uint32_t psk_word(float v)
{
#pragma clang fp contract(off)
    float f = v * 683565275.57643158f;                    // 2^31 / pi, rounded to f32 by the compiler
    if (!(f == f)) f = 0.0f;
    f = f > 1073741824.0f ? 1073741824.0f : (f < -1073741824.0f ? -1073741824.0f : f);
    return (uint32_t)(int32_t)rintf(f);
}

}  // namespace csdr
