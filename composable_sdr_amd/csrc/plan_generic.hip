// The any-M route of the chain (the last RouteRow of capi.hip) as a ChainPlan: DC blocker + pre-mix, polyphase FIR, DFT and the
// frame-major FM / mix endings as separate kernels (kernels_generic.hip, kernels_dc_tile.hip, k_pfb1024), for any channel count,
// any shard and any DC-blocker alpha; M = 1 is the DC blocker [+ freqdem] alone.  Host code only.  Product code.
#include "../../include/csdr.h"
#include "fused.h"

#include <cmath>
#include <optional>

namespace csdr {
namespace {

struct GenericPlan : ChainPlan {
    using ChainPlan::ChainPlan;
    std::string kernel;              // the timed kernel: the create-time choice until a call times another one
    uint32_t tab_len = 0;            // period of the pre-mix phase sequence (0: too long for a table, sincos on the device)
    float *d_taps = nullptr;
    float2 *d_tw = nullptr, *d_nco_tab = nullptr, *d_dcstate = nullptr, *d_scratch = nullptr;
    float2 *d_tw_g = nullptr, *d_fold_ph = nullptr, *d_fold = nullptr;   // interleaved shard (pruned DFT): (M/G)-point twiddles, fold phasors, folded frames
    std::optional<DcTilePlan> dctile;    // DC blocker with an alpha the single-pass scan kernel takes; none: launch_dc_mix (+dc-scan)
    bool use1024 = false;            // M = 1024: FIR + DFT + transpose [+ freqdem] in k_pfb1024
    bool mix_identity = false;       // DeNo --mix over all channels: M * (branch-0 FIR) instead of bank + DFT + sum
    bool mix_identity_shard = false; // the same for an interleaved shard g of G: (M / G) * sum of the G surviving branches' FIRs
    float2 *d_u0 = nullptr, *d_u0hist = nullptr;     // branch-0 samples of the call behind p - 1 of history; history between calls (two copies, ping-pong)
    float2 *d_u = nullptr, *d_hist_tmp = nullptr;    // pre-mixed input behind (p - 1) frames of history
    float2 *d_A = nullptr, *d_B = nullptr;           // FIR plane X[nf][M] (M = 1 with freqdem: Z); DFT plane Y (k_pfb1024: yfirst | ylast)
    float2 *d_rp[2] = {nullptr, nullptr};            // cfg.fm: freqdem history r' per channel, ping-pong

    int init();
    // one kernel sequence per handle, no choice by call size; the name is what init() and run() noted in `kernel`
    KernelChoice choose(uint32_t) const override { return {}; }
    const char *kernel_name(int) const override { return kernel.c_str(); }
    std::string route(const char *, bool) const override;
    bool tile_major_ok(uint32_t) const override { return false; }
    int status(unsigned *st) override { *st = 0; return dctile ? dctile->status(st) : 0; }
    int reset_state(hipStream_t s) override;
    int run(const FusedCall &call, KernelChoice, void *out, hipStream_t s, KernelTimer *timer) override;
    int run_mix_identity(const FusedCall &call, const NcoParams &nco, hipStream_t s, KernelTimer *timer);
};

std::string GenericPlan::route(const char *, bool) const
{
    std::string t = use1024 ? "generic+pfb1024" : (mix_identity ? "generic+mix-identity" : "generic");
    if (cfg.G > 1) t = mix_identity_shard ? "generic+pruned-dft+shard-mix-identity" : "generic+pruned-dft";
    if (cfg.M > 1 && cfg.dc_block && !dctile) t += "+dc-scan";     // alpha outside the DC shortcuts (dc_window_ok): launch_dc_mix
    return t;
}

int GenericPlan::init()
{
    const uint32_t M = cfg.M, p = cfg.p, C = cfg.C, G = cfg.G;
    const uint64_t max_nx = (uint64_t)cfg.max_nf * M;
    const double tp = -2.0 * 3.14159265358979323846;
    int r;
    if ((r = mem.alloc_n(&d_dcstate, 1)) || (r = mem.alloc_n(&d_scratch, 2 * (size_t)(max_nx / DC_BLOCK + 2)))) return r;
    if (cfg.fm && ((r = mem.alloc_n(&d_rp[0], C)) || (r = mem.alloc_n(&d_rp[1], C)))) return r;
    if (M == 1) {
        kernel = "k_dc_apply";
        return cfg.fm ? mem.alloc_n(&d_A, max_nx) : 0;
    }
    tab_len = nco_period(cfg.d_theta, 1u << 17);
    if ((r = mem.alloc_n(&d_taps, (size_t)M * p))) return r;
    CSDR_HIP(hipMemcpy(d_taps, cfg.taps, sizeof(float) * M * p, hipMemcpyHostToDevice));
    if (tab_len) {
        std::vector<float2> tab(tab_len);
        for (uint32_t i = 0; i < tab_len; i++) { float c, s; nco_phasor(i * cfg.d_theta, &c, &s); tab[i] = make_float2(c, s); }
        if ((r = mem.alloc_n(&d_nco_tab, tab_len))) return r;
        CSDR_HIP(hipMemcpy(d_nco_tab, tab.data(), sizeof(float2) * tab_len, hipMemcpyHostToDevice));
    }
    std::vector<float2> tw(M);
    for (uint32_t i = 0; i < M; i++) tw[i] = make_float2((float)std::cos(tp * (double)i / (double)M), (float)std::sin(tp * (double)i / (double)M));
    if ((r = mem.alloc_n(&d_tw, M))) return r;
    CSDR_HIP(hipMemcpy(d_tw, tw.data(), sizeof(float2) * M, hipMemcpyHostToDevice));

    use1024 = G == 1 && pfb1024_supported(M, p) && !cfg.mix && !diag_env("CSDR_NO_PFB1024");
    kernel = use1024 ? "k_pfb1024" : "k_pfb_fir";
    const size_t hist = (size_t)(p - 1) * M;
    if ((r = mem.alloc_n(&d_u, hist + max_nx)) || (r = mem.alloc_n(&d_hist_tmp, hist))) return r;
    if ((r = mem.alloc_n(&d_A, max_nx)) || (r = mem.alloc_n(&d_B, use1024 && max_nx < 2048 ? 2048 : max_nx))) return r;   // k_pfb1024 keeps yfirst|ylast (2 x nruns x 1024) in d_B
    const bool tile = cfg.dc_block && dctile_supported(cfg.dc);
    const bool deno_mix = cfg.mix && !cfg.fm && tile && !cfg.no_mix_identity;       // (cfg.mix, cfg.fm: without the AGC)
    mix_identity = deno_mix && G == 1 && C == M;
    if (mix_identity) {
        if ((r = mem.alloc_n(&d_u0, (size_t)(p - 1) + cfg.max_nf)) || (r = mem.alloc_n(&d_u0hist, 2 * (p - 1)))) return r;
        kernel = (M % 4096u == 0) ? "k_dc_fold" : "k_dc_tile";   // refined per call
    }
    // interleaved shard, DeNo --mix, no AGC: only the G branches (M / G) n2 survive the shard's channel sum (kernels_dc_tile.hip, k_dc_fold8)
    // (the conditions of DcTilePlan::mix_identity_shard_supported that do not depend on the call: every call of whole frames then takes it)
    mix_identity_shard = deno_mix && (G == 2 || G == 4 || G == 8) && (uint64_t)C * G == M && M % 4096u == 0 && (M / G) % 512u == 0 &&
                         p <= 33u && cfg.dc.beta > 0.f;
    if (tile && (r = dctile.emplace(cfg.dc).init(mem, max_nx, cus, mix_identity_shard))) return r;
    if (mix_identity_shard && (r = mem.alloc_n(&d_u0hist, 2 * (size_t)(p - 1) * G))) return r;
    if (G > 1) {
        const uint32_t Mg = M / G, c0 = cfg.c0;
        std::vector<float2> twg(Mg), ph(G + Mg);
        for (uint32_t i = 0; i < Mg; i++) twg[i] = make_float2((float)std::cos(tp * i / Mg), (float)std::sin(tp * i / Mg));
        for (uint32_t j2 = 0; j2 < G; j2++) ph[j2] = make_float2((float)std::cos(tp * ((uint64_t)j2 * c0 % G) / G), (float)std::sin(tp * ((uint64_t)j2 * c0 % G) / G));
        for (uint32_t j1 = 0; j1 < Mg; j1++) ph[G + j1] = make_float2((float)std::cos(tp * ((uint64_t)j1 * c0 % M) / M), (float)std::sin(tp * ((uint64_t)j1 * c0 % M) / M));
        if ((r = mem.alloc_n(&d_tw_g, Mg)) || (r = mem.alloc_n(&d_fold_ph, G + Mg)) || (r = mem.alloc_n(&d_fold, (size_t)Mg * cfg.max_nf))) return r;
        if (hipMemcpy(d_tw_g, twg.data(), sizeof(float2) * Mg, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_fold_ph, ph.data(), sizeof(float2) * (G + Mg), hipMemcpyHostToDevice) != hipSuccess) { set_error("chain: fold table upload failed"); return CSDR_ERR_HIP; }
        if (mix_identity_shard) kernel = "k_dc_fold8";
    }
    return 0;
}

int GenericPlan::reset_state(hipStream_t s)
{
    CSDR_HIP(hipMemsetAsync(d_dcstate, 0, sizeof(float2), s));
    if (d_u) CSDR_HIP(hipMemsetAsync(d_u, 0, sizeof(float2) * (size_t)(cfg.p - 1) * cfg.M, s));
    if (d_u0hist) CSDR_HIP(hipMemsetAsync(d_u0hist, 0, sizeof(float2) * 2 * (cfg.p - 1) * (mix_identity_shard ? cfg.G : 1u), s));
    for (float2 *rp : d_rp) if (rp) CSDR_HIP(hipMemsetAsync(rp, 0, sizeof(float2) * cfg.C, s));
    return dctile ? dctile->reset(s) : 0;
}

// DeNo --mix without computing the bank: the channel sum of a frame from the surviving polyphase branches (histories: ping-pong by cur)
int GenericPlan::run_mix_identity(const FusedCall &call, const NcoParams &nco, hipStream_t s, KernelTimer *timer)
{
    const uint32_t M = cfg.M, p = cfg.p, nf = call.nf, nx = nf * M;
    float2 *out = (float2 *)call.d_out;
    int r;
    if (mix_identity_shard) {
        // the shard's channel sum = (M / G) x sum of the G surviving branches' FIRs.  The create-time predicate holds every condition
        // that does not depend on the call, and calls are whole frames: a call it refuses is a bug, not a reason to switch routes (the
        // pruned-DFT route keeps no branch histories of its own)
        if (!dctile->mix_identity_shard_supported(M, nx, p, cfg.G)) { set_error("chain: shard mix identity refused a call of %u samples", nx); return CSDR_ERR_INVALID; }
        const size_t hs = (size_t)(p - 1) * cfg.G;
        kernel = "k_dc_fold8";
        if (timer && (r = timer->begin(s))) return r;
        if ((r = dctile->mix_identity_shard(call.d_in, nx, nco, d_nco_tab, d_taps, M, p, cfg.G, cfg.c0, d_u0hist + (size_t)cur * hs, d_u0hist + (size_t)(cur ^ 1) * hs, out, s))) return r;
        return timer ? timer->end(s) : 0;
    }
    // sum over ALL channels of a frame = M * X_t[0]: DC blocker + pre-mix on the whole stream, every M-th sample kept,
    // then the 2m-tap FIR of polyphase branch 0 (no bank, no DFT, no channel sum; 8 B read per input sample)
    float2 *hin = d_u0hist + (size_t)cur * (p - 1), *hout = d_u0hist + (size_t)(cur ^ 1) * (p - 1);
    if (dctile->mix_identity_supported(M, nx, p)) {
        // k_dc_fold (one aggregate per tile: a plain streaming read) + k_mixid_finish (DC state, pick, pre-mix, FIR)
        kernel = "k_dc_fold";
        if (timer && (r = timer->begin(s))) return r;
        if ((r = dctile->mix_identity(call.d_in, nx, nco, d_nco_tab, d_taps, M, p, hin, hout, out, s))) return r;
        return timer ? timer->end(s) : 0;
    }
    kernel = "k_dc_tile";
    CSDR_HIP(hipMemcpyAsync(d_u0, hin, sizeof(float2) * (p - 1), hipMemcpyDeviceToDevice, s));
    if (timer && (r = timer->begin(s))) return r;
    if ((r = dctile->process(call.d_in, d_u0 + (p - 1), nx, true, nco, d_nco_tab, s, M))) return r;
    if (timer && (r = timer->end(s))) return r;
    return launch_branch0_fir(d_u0, d_taps, out, hout, M, p, nf, s);
}

// With the AGC on (cfg.fm and cfg.mix are then false) out receives the channel-major CF32 plane the handle's tail reads
int GenericPlan::run(const FusedCall &call, KernelChoice, void *out, hipStream_t s, KernelTimer *timer)
{
    const uint32_t M = cfg.M, C = cfg.C, G = cfg.G, nf = call.nf, nx = nf * M;
    const float2 *rp_in = d_rp[cur]; float2 *rp_out = d_rp[cur ^ 1];
    int r;
    NcoParams nco{};
    if (M == 1) {
        float2 *Z = cfg.fm ? d_A : (float2 *)out;
        if (timer && (r = timer->begin(s))) return r;
        if ((r = launch_dc_mix(call.d_in, Z, nx, cfg.dc_block, cfg.dc, d_dcstate, d_scratch, false, nco, nullptr, s))) return r;
        if (timer && (r = timer->end(s))) return r;
        return cfg.fm ? launch_fm(Z, (float *)out, C, nf, cfg.fm_ref, rp_in, rp_out, s) : 0;
    }
    nco.theta0 = call.theta0; nco.d_theta = cfg.d_theta; nco.tab_len = tab_len; nco.up = 0;
    nco.tab_pos = tab_len ? (uint32_t)(frames_done * M % tab_len) : 0;
    if (mix_identity || mix_identity_shard) return run_mix_identity(call, nco, s, timer);
    const size_t hist = (size_t)(cfg.p - 1) * M;
    float2 *u_new = d_u + hist;
    if (dctile) r = dctile->process(call.d_in, u_new, nx, true, nco, d_nco_tab, s);
    else r = launch_dc_mix(call.d_in, u_new, nx, cfg.dc_block, cfg.dc, d_dcstate, d_scratch, true, nco, d_nco_tab, s);
    if (r) return r;
    // M = 1024: FIR + DFT + transpose [+ freqdem] in one kernel (no X / Y round trips through HBM); the frame-major
    // mix endings still want Y in HBM and keep the three-kernel route
    if (timer && (r = timer->begin(s))) return r;
    if (use1024) r = launch_pfb1024(u_new, d_taps, d_tw, out, cfg.fm, nf, cfg.c0, C, cfg.fm_ref, cfg.fm ? rp_in : nullptr, cfg.fm ? rp_out : nullptr, d_B, cus, s);
    else r = launch_pfb_fir(u_new, d_taps, d_A, M, cfg.p, nf, s);
    if (r) return r;
    if (timer && (r = timer->end(s))) return r;
    // keep the last (p-1) frames of premixed input as the next call's history
    CSDR_HIP(hipMemcpyAsync(d_hist_tmp, d_u + nx, sizeof(float2) * hist, hipMemcpyDeviceToDevice, s));
    CSDR_HIP(hipMemcpyAsync(d_u, d_hist_tmp, sizeof(float2) * hist, hipMemcpyDeviceToDevice, s));
    if (use1024) return 0;
    const uint32_t Mw = M / G, cw = G > 1 ? 0u : cfg.c0;     // width of a DFT output frame, first owned bin in it
    if (G > 1) {
        // interleaved shard: fold the G sub-blocks of every frame, then an (M/G)-point DFT: d_B = Y[t][c0 + G m]
        if ((r = launch_fold(d_A, d_fold, d_fold_ph, M, G, nf, s))) return r;
        r = launch_dft(d_fold, d_B, d_tw_g, Mw, nf, s);
    } else if (cfg.mix && !cfg.fm && C == M && dft_mix_supported(M)) {
        // DeNo --mix over all channels: the frame sum happens inside the DFT kernel, Y never goes to HBM
        return launch_dft_mix(d_A, (float2 *)out, d_tw, M, nf, s);
    } else r = launch_dft(d_A, d_B, d_tw, M, nf, s);
    if (r) return r;
    // frame-major endings: no transpose in front of freqdem / mix
    if (cfg.mix) return launch_mix_frames(d_B, out, cfg.fm, Mw, nf, cw, C, cfg.fm_ref, rp_in, rp_out, s);
    if (cfg.fm) return launch_transpose_fm(d_B, (float *)out, Mw, nf, cw, C, cfg.fm_ref, rp_in, rp_out, s);
    return launch_transpose(d_B, (float2 *)out, Mw, nf, cw, C, s);
}

}  // namespace

bool generic_supported(uint32_t, uint32_t) { return true; }
int generic_create(const FusedConfig &cfg, ChainPlan **out) { return make_plan<GenericPlan>(cfg, out); }

}  // namespace csdr
