// What the chain plans share (fused.h): the call sequence of ChainPlan (one kernel choice per call), the carried stream state, the DC
// blocker's constants and the set-up of cold starts without warm-up windows.  Host code only.  Product code.
#include "fused.h"

#include <cmath>
#include <cstdio>

namespace csdr {

int ChainPlan::process(const FusedCall &call, hipStream_t s, KernelTimer *timer)
{
    if (!call.nf) return 0;
    if ((call.tile_major && !tile_major_ok(call.nf)) || (call.indep && !can_overlap(call.nf))) {
        set_error("fused: internal: tile-major output or an independent launch requested from a call that cannot run as one");
        return -1;
    }
    last = choose(call.nf);
    int r = run(call, last, d_premix ? d_premix : call.d_out, s, timer);
    if (r) return r;
    cur ^= 1;
    frames_done += call.nf;
    if (d_premix) return launch_mix((const float *)d_premix, (float *)call.d_out, cfg.C, cfg.fm ? call.nf : 2 * call.nf, s);
    return 0;
}

std::vector<float2> ChainPlan::premix_table() const
{
    std::vector<float2> wpre(2 * cfg.M);
    for (uint32_t i = 0; i < 2 * cfg.M; i++) {
        float c, s;
        nco_phasor(i * cfg.d_theta, &c, &s);
        wpre[i] = make_float2(c, -s);
    }
    return wpre;
}

int StreamState::alloc(DeviceBuffers &mem, size_t nh, size_t nr)
{
    int r;
    n_hist = nh; n_rp = nr;
    for (int i = 0; i < 2; i++)
        if ((r = mem.alloc_n(&hist[i], n_hist)) || (r = mem.alloc_n(&vend[i], 1)) || (r = mem.alloc_n(&rp[i], n_rp))) return r;
    return 0;
}

int StreamState::reset(hipStream_t s) const
{
    for (int i = 0; i < 2; i++) {
        CSDR_HIP(hipMemsetAsync(hist[i], 0, sizeof(float2) * n_hist, s));
        CSDR_HIP(hipMemsetAsync(vend[i], 0, sizeof(float2), s));
        CSDR_HIP(hipMemsetAsync(rp[i], 0, sizeof(float2) * n_rp, s));
    }
    return 0;
}

DcConsts::DcConsts(bool dc_block, const DcParams &dc)
{
    const double b = dc_block ? (double)dc.beta : 0.0;
    alpha = dc_block ? (float)(1.0 - b) : 0.0f;    // alpha = 1 - beta with beta = f32(1 - 0.0005)
    beta = (float)b;
    l2beta = dc_block ? (float)std::log2(b) : -1000.0f;
    for (int k = 0; k < 16; k++) b16[k] = (float)std::pow(b, 16.0 * k);
    for (int k = 0; k < 17; k++) b256[k] = (float)std::pow(b, 256.0 * k);
    for (int k = 0; k < 16; k++) bj[k] = (float)std::pow(b, (double)k);
    for (int k = 0; k < 12; k++) wtile[k] = (float)std::pow(b, 4096.0 * k);
}

int ColdStart::init(DeviceBuffers &mem, const FusedConfig &cfg, double window, uint32_t max_runs, size_t side_per_run, bool state_always,
                    uint32_t f0, uint32_t nfr, int k0, const float2 *wpre)
{
    int r;
    runs = max_runs;
    const size_t n_cpre = (size_t)max_runs + 2, n_side = ((size_t)max_runs + 1) * side_per_run;
    const char *e = diag_env("CSDR_NOWU");
    const bool on = cfg.dc_block && dc_window_ok(cfg.dc, window) && !(e && atoi(e) == 0);
    if (on || state_always) {
        if ((r = mem.alloc_n(&cpre, n_cpre)) || (n_side && (r = mem.alloc_n(&side, n_side)))) return r;
        CSDR_HIP(hipMemset(cpre, 0, sizeof(float2) * n_cpre));
    }
    if (!on) return 0;
    std::vector<float2> t((size_t)2 * nfr * 4, make_float2(0.f, 0.f));
    if (k0 >= 0) dc_state_response(cfg, wpre, f0, nfr, (uint32_t)k0, t.data());
    if ((r = mem.alloc_n(&rt, t.size()))) return r;
    CSDR_HIP(hipMemcpy(rt, t.data(), sizeof(float2) * t.size(), hipMemcpyHostToDevice));
    return 0;
}

void dc_state_response(const FusedConfig &cfg, const float2 *wpre, uint32_t f0, uint32_t nfr, uint32_t k0, float2 *rt)
{
    // the blocker's output carries -alpha beta^n of the state at sample n behind the tile's start; that goes through the pre-mix, the
    // polyphase FIR and the DFT like any input
    const uint32_t M = cfg.M, T = f0 + nfr;
    const double beta = (double)cfg.dc.beta, alpha = 1.0 - beta, tp = -2.0 * 3.14159265358979323846;
    std::vector<double> ur((size_t)T * M), ui((size_t)T * M), xr(M), xi(M);
    for (uint32_t par = 0; par < 2; par++) {
        for (uint32_t f = 0; f < T; f++)
            for (uint32_t j = 0; j < M; j++) {
                const double e = -alpha * std::pow(beta, (double)f * M + j);
                const float2 wv = wpre[((par + f) & 1u) * M + j];
                ur[(size_t)f * M + j] = e * (double)wv.x; ui[(size_t)f * M + j] = e * (double)wv.y;
            }
        for (uint32_t t = 0; t < nfr; t++) {
            const uint32_t f = f0 + t;
            for (uint32_t j = 0; j < M; j++) {
                double ar = 0.0, ai = 0.0;
                for (uint32_t n = 0; n < cfg.p && n <= f; n++) {
                    const double hh = (double)cfg.taps[(M - 1 - j) + n * M];
                    ar += hh * ur[(size_t)(f - n) * M + j]; ai += hh * ui[(size_t)(f - n) * M + j];
                }
                xr[j] = ar; xi[j] = ai;
            }
            for (uint32_t ch = 0; ch < 4; ch++) {
                const uint32_t k = k0 + ch;
                double yr = 0.0, yi = 0.0;
                for (uint32_t j = 0; j < M; j++) {
                    const double a = tp * (double)((j * k) % M) / (double)M, cr = std::cos(a), ci = std::sin(a);
                    yr += xr[j] * cr - xi[j] * ci; yi += xr[j] * ci + xi[j] * cr;
                }
                rt[((size_t)par * nfr + t) * 4 + ch] = make_float2((float)yr, (float)yi);
            }
        }
    }
}

}  // namespace csdr
