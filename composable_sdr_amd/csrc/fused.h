// Interface between the chain handle of the C ABI (capi.hip) and the plans of its routes: the four fused channelizers (M = 64, 256,
// 1024, 4096) and the any-M route.  Product code.
//   chain_plan.cpp            what the plans share: ChainPlan::process, StreamState, DcConsts, ColdStart, dc_state_response
//   kernel_choice.h           which kernel a call takes (KernelChoice, the run counts, the M = 64 and M = 1024 selection) and whether
//                             its runs start cold (the run-length rules); no HIP
//   run_split.h               the bounds of run w for every run kernel, and the constants they are judged against; no HIP
//   agc_tail_shape.h          the launch shape of the AGC tail behind the plans (kernels_agc_tail.hip, chain_tails.h); no HIP
//   kernels_fused_small.hip   M = 64: SmallPlan, k_run64; its run kernel k_run64v2 in kernels_run64_v2.hip
//   kernels_fused.hip         M = 256: FusedPlan, k_tile256; its run kernel k_run256v2 in kernels_fused_v2.hip
//   kernels_pfb1024.hip       M = 1024: BigPlan, k_run1024; its run kernels in kernels_run1024_v2.hip, kernels_run1024_v3.hip, kernels_shard1024.hip
//   kernels_pfb4096.hip       M = 4096: HugePlan, k_front4096 + k_back4096
//   plan_generic.hip          any M: GenericPlan over kernels_generic.hip, kernels_dc_tile.hip and k_pfb1024
#pragma once
#include "csdr_internal.h"
#include "kernel_choice.h"
#include <type_traits>
#include <utility>

namespace csdr {

struct FusedConfig {
    uint32_t M, p, C, c0, max_nf;
    uint32_t G = 1;          // > 1: interleaved shard c0 of G (channels c0, c0 + G, ...; C = M / G rows out): k_run256v2<.., G>, G = 2, 4, 8
    bool dc_block; DcParams dc;
    bool fm; float fm_ref;
    bool mix;
    const float *taps;       // host, M*p
    uint32_t d_theta;
    uint32_t cus = 256;      // compute units of the device (the run counts of the launches)
    bool no_mix_identity = false;    // CSDR_FLAG_NO_MIX_IDENTITY (any-M route: DeNo --mix through the full bank + DFT + sum)
};

struct FusedCall {
    const float2 *d_in;      // nf*M new samples
    void *d_out;             // [C][nf] CF32 / F32, or [nf] when mixing
    uint32_t nf;
    uint32_t theta0;         // NCO phase of the first sample
    // pipelined entry point (csdr_chain_submit_device): run the launch without reading anything an earlier launch wrote, if the
    // plan can (ChainPlan::can_overlap); ev_tail is recorded on s once the chunk's last tiles are saved for the next call's run 0
    bool indep = false;
    hipEvent_t ev_tail = nullptr;
    // CF32 plans: write the output TILE-MAJOR -- block t / 16 holds the 128-byte lines of all C rows back to back (a tile's whole
    // output is one contiguous C x 128 bytes) -- instead of row-major [C][nf]: what the time-parallel AGC tail reads (k_agc_spec_tm).
    // Only for calls ChainPlan::tile_major_ok() accepts.
    bool tile_major = false;
};

// What the plans share lives in chain_plan.cpp.
// The stream state the 64-, 256- and 1024-channel plans carry between calls, as ping-pong pairs: a call reads the side [cur] and writes
// [cur ^ 1].  hist: the 13 frames in front of the call (DC-blocked samples), vend: the DC blocker's v1, rp: freqdem's r' per channel.
struct StreamState {
    int alloc(DeviceBuffers &mem, size_t n_hist, size_t n_rp);
    int reset(hipStream_t s) const;      // zero both sides
    const float2 *hist_in(int cur) const { return hist[cur]; }      float2 *hist_out(int cur) const { return hist[cur ^ 1]; }
    const float2 *vend_in(int cur) const { return vend[cur]; }      float2 *vend_out(int cur) const { return vend[cur ^ 1]; }
    const float2 *rp_in(int cur) const { return rp[cur]; }          float2 *rp_out(int cur) const { return rp[cur ^ 1]; }
private:
    float2 *hist[2] = {nullptr, nullptr}, *vend[2] = {nullptr, nullptr}, *rp[2] = {nullptr, nullptr};
    size_t n_hist = 0, n_rp = 0;
};

// The DC blocker's constants as the kernels take them (v[n] = x[n] + beta v[n-1], y = x - alpha v[n-1]): fixed when the plan is made.
// Blocker off: beta = 0 (every power but the zeroth is 0) and l2beta = -1000.
struct DcConsts {
    float alpha, beta, l2beta;      // alpha = 1 - beta with beta = f32(1 - alpha of the handle); log2(beta)
    float b16[16], b256[17], bj[16], wtile[12];      // beta^(16 i), beta^(256 i), beta^i, beta^(4096 i) (LOOKBACK + 2 tiles: fused_common.h)
    DcConsts(bool dc_block, const DcParams &dc);
    // into the members of a kernel's argument struct that carry them (every struct has alpha; the rest as declared)
    template <class Args> void put(Args &A) const
    {
        A.alpha = alpha;
        if constexpr (has_beta<Args>::value) A.beta = beta;
        if constexpr (has_l2beta<Args>::value) A.l2beta = l2beta;
        if constexpr (has_b16<Args>::value) { copy(A.b16, b16); copy(A.b256, b256); }
        if constexpr (has_bj<Args>::value) { copy(A.bj, bj); copy(A.wtile, wtile); }
    }
private:
#define CSDR_HAS_MEMBER(m)                                                                                                       \
    template <class A, class = void> struct has_##m : std::false_type {};                                                        \
    template <class A> struct has_##m<A, std::void_t<decltype(std::declval<A &>().m)>> : std::true_type {};
    CSDR_HAS_MEMBER(beta) CSDR_HAS_MEMBER(l2beta) CSDR_HAS_MEMBER(b16) CSDR_HAS_MEMBER(bj)
#undef CSDR_HAS_MEMBER
    template <size_t N> static void copy(float (&dst)[N], const float (&src)[N]) { for (size_t i = 0; i < N; i++) dst[i] = src[i]; }
};

// Cold starts without warm-up windows: a run starts its halo tile from DC state 0 and a correction kernel behind the launch puts
// back, at the four channels around DC, what the true state would have added.  cpre: the state hand-over between the runs; side: the
// uncorrected samples of those channels; rt: [2 parities][nfr][4] the chain's response to a unit state (dc_state_response), null when the
// handle keeps its warm-up windows (blocker off, an alpha the window does not fit: dc_window_ok, or CSDR_NOWU=0).
struct ColdStart {
    float2 *cpre = nullptr, *side = nullptr, *rt = nullptr;
    uint32_t runs = 0;          // launches of up to this many runs fit the arrays
    // window: the samples behind a cold start after which the missing state is dropped.  cpre (max_runs + 2 elements, zeroed) and side
    // (max_runs + 1 runs of side_per_run elements; 0: none) are made with rt, or whatever rt when state_always (kernels that write them on
    // every launch).  rt: frames f0 .. f0 + nfr - 1 behind the tile's start at the channels k0 .. k0 + 3 on the phasor table wpre (k0 < 0:
    // all zero)
    int init(DeviceBuffers &mem, const FusedConfig &cfg, double window, uint32_t max_runs, size_t side_per_run, bool state_always,
             uint32_t f0, uint32_t nfr, int k0, const float2 *wpre);
    // the capacity half of a call's cold-start decision (the shape half: kernel_choice.h): the handle runs without warm-up windows and a
    // launch of nruns runs fits the arrays
    bool fits(uint32_t nruns) const { return rt && cold_fits(runs, nruns); }
};

// The plan of one route (a RouteRow of capi.hip): M = 64 (kernels_fused_small.hip), 256 (kernels_fused.hip), 1024 (kernels_pfb1024.hip),
// 4096 (kernels_pfb4096.hip) and any M (plan_generic.hip) derive from it.  With the AGC on (cfg.fm and cfg.mix are then false) a plan delivers
// the channel-major CF32 plane the handle's tail reads; without it, the call's output.  The base owns what they share: the configuration, the CU count, the global frame counter,
// the ping-pong index of the state buffers, the device buffers (mem: freed with the plan), the mix ending of the 64, 256 and 1024 plans
// (run() writes d_premix, process() sums its rows into the call's output) and the kernel choice of the last call: a plan answers "which
// kernel does a call of nf frames take, with how many runs" in choose() alone; process() asks once per call, hands the answer to run()
// and keeps it for name() and route(); tile_major_ok() and can_overlap() are predicates on the same answer.
struct ChainPlan {
    FusedConfig cfg;
    uint32_t cus;                // compute units the launches are sized for (cfg.cus; the M = 256 plan takes CSDR_CUS)
    uint64_t frames_done = 0;    // global frame index of the next frame (its parity selects the pre-mix phasor row)
    int cur = 0;                 // the next call reads the state buffers [cur] and writes [cur ^ 1]
    void *d_premix = nullptr;    // per-channel output in front of launch_mix (cfg.mix; the M = 4096 plan mixes in its back kernel)
    DeviceBuffers mem;
    const DcConsts dcc;          // of cfg.dc_block and cfg.dc
    KernelChoice last;           // of the last call (make_plan: first_choice() until then)

    explicit ChainPlan(const FusedConfig &c) : cfg(c), cus(c.cus), dcc(c.dc_block, c.dc) {}
    virtual ~ChainPlan() = default;

    // One call.  A tile-major or independent request the plan cannot run (tile_major_ok, can_overlap) is refused before anything is queued.
    int process(const FusedCall &call, hipStream_t s, KernelTimer *timer);
    int reset(hipStream_t s) { cur = 0; frames_done = 0; return reset_state(s); }
    void seek(uint64_t frames) { frames_done = frames; }     // after reset: global frame index of the next frame
    // The kernel a call of nf frames takes: a function of cfg, the knobs init() read, cus and nf, nothing else (no stream state)
    virtual KernelChoice choose(uint32_t nf) const = 0;
    // the kernel the last call launched (before the first call: first_choice())
    const char *name() const { return kernel_name(last.id); }
    // csdr_chain_path in front of the handle's tails (+am, +wbfm, +dft-backward, -spec); prefix: the RouteRow's
    virtual std::string route(const char *prefix, bool agc) const
    {
        return std::string(prefix) + name() + (cfg.G > 1 ? "+interleaved-shard" : "") + (agc ? "+agc" : "");
    }
    virtual bool tile_major_ok(uint32_t nf) const = 0;     // FusedCall::tile_major for a call of nf frames

    // M = 256 only
    virtual void keep_tail() {}                                 // from now on every run-kernel call saves its last WU + 1 raw tiles
    virtual bool can_overlap(uint32_t nf) const { (void)nf; return false; }    // the next call of nf frames can run with FusedCall::indep
    virtual bool tail_recorded() const { return false; }        // the last call saved its tail (and recorded FusedCall::ev_tail)
    // sticky device-side error word (bit0/bit1: an inter-workgroup wait hit its spin limit); reads, then clears it; synchronises
    virtual int status(unsigned *st) { *st = 0; return 0; }
    // CSDR_TRACE=1: per-tile s_memtime stamps (16 per tile) of the last launches; returns tiles copied
    virtual int trace(unsigned long long *out, uint32_t ntiles) { (void)out; (void)ntiles; return 0; }

protected:
    // nco_crcf_mix_block_down's phasor conj(cos + j sin) of theta = n d_theta, n < 2M: the phase sequence has period 2M for a power-of-two M
    // (row 0: even frames, n = j; row 1: odd frames, n = M + j)
    std::vector<float2> premix_table() const;
    virtual int reset_state(hipStream_t s) = 0;      // zero the stream state the plan carries between calls
    virtual const char *kernel_name(int id) const = 0;      // the plan's table: KernelChoice::id -> text
    // what name() says before the first call: the kernel a call of max_nf frames takes (M = 64, 256: their first kernel, as their paths always read)
    virtual KernelChoice first_choice() const { return choose(cfg.max_nf); }
    // the call's launches, kernel k = choose(call.nf), into out (d_premix when mixing); a launch sequence with two steps may flip cur between them,
    // process() flips it behind the call
    virtual int run(const FusedCall &call, KernelChoice k, void *out, hipStream_t s, KernelTimer *timer) = 0;
    template <class Plan> friend int make_plan(const FusedConfig &cfg, ChainPlan **out);
};

// the factories' common part: a plan of type Plan, set up by its init()
template <class Plan> int make_plan(const FusedConfig &cfg, ChainPlan **out)
{
    Plan *p = new Plan(cfg);
    if (int r = p->init()) { delete p; return r; }
    p->last = p->first_choice();
    *out = p;
    return 0;
}

// One route per channel count (RouteRow, capi.hip): whether the plan takes M channels of p taps per branch, and the factory
bool plan256_supported(uint32_t M, uint32_t p);
int  plan256_create(const FusedConfig &cfg, ChainPlan **out);
bool plan64_supported(uint32_t M, uint32_t p);
int  plan64_create(const FusedConfig &cfg, ChainPlan **out);
bool plan1024_supported(uint32_t M, uint32_t p);      // (CSDR_NO_RUN1024: no)
int  plan1024_create(const FusedConfig &cfg, ChainPlan **out);
// M = 4096: branch-tiled front kernel (DC blocker + pre-mix + FIR + first radix-4 stage) -> z -> back kernel (four 1024-point DFTs per
// frame + tails); whole band
bool plan4096_supported(uint32_t M, uint32_t p);      // (CSDR_NO_RUN4096: no)
int  plan4096_create(const FusedConfig &cfg, ChainPlan **out);
// any M, any shard, any alpha (plan_generic.hip): what no row above takes
bool generic_supported(uint32_t M, uint32_t p);
int  generic_create(const FusedConfig &cfg, ChainPlan **out);

// second-generation run kernel of the M = 256 chain (kernels_fused_v2.hip): whole-band calls of >= run_min_tiles tiles.
// run_args points at a RunArgs (fused_common.h) the plan fills.
int  run256_v2_launch(const void *run_args, bool fm, unsigned G, unsigned nruns, hipStream_t s);
int  run256_v2_blocks_per_cu(bool fm, unsigned G);
// RunArgs::nowu launches: the near-DC channels of every run's first 112 frames get what the true DC state at the run's start adds (Rt: host table
// [2 parities][DCFIX_F][4], fused_common.h)
int  run256_dcfix_launch(const void *run_args, bool fm, unsigned nruns, const float2 *Rt, hipStream_t s);


// k_run64v2 (kernels_run64_v2.hip): whole-band M = 64 calls with CF32 output and nf % 64 == 0; same state buffers as k_run64
struct Run64v2Host {
    const float2 *x; float2 *out;
    const float *taps; const float2 *tw, *wpre;
    const float2 *uhist_in; float2 *uhist_out; const float2 *vend_in; float2 *vend_out;
    // runs without warm-up windows (round 5, as k_run256v2: DESIGN 4): cpre [nruns + 1] DC state in front of every run's halo tile,
    // rt [2 parities][RUN64_DCFIX_F][4] the chain's response to a unit state at the channels 30..33; cold: this call's runs start that
    // way (ColdStart::fits and run64_v2_cold, combined by the plan); else warm-up windows
    float2 *cpre = nullptr; const float2 *rt = nullptr; bool cold = false;
    uint32_t nf, nruns, parity0;
    uint32_t G = 1, g = 0;      // interleaved shard g of G (tables rotated by the plan)
    bool tile_major = false;    // CF32 plane of the AGC route: [block of 16 frames][64][128 B]
    const DcConsts *dc;         // the plan's
    double weight = 1.1;        // tile share of the older workgroup of a CU (1 = even; 1.1 measured best: 243 vs 250 us; CSDR_RUN64_WEIGHT)
};
// Response of the chain (pre-mix table wpre [2][M], taps, forward DFT), at the channels k0 .. k0 + 3, to a DC-blocker state of 1 in
// front of a tile: frames f0 .. f0 + nfr - 1 behind the tile's start, both parities of the tile's first frame; rt [2][nfr][4], f64 inside
void dc_state_response(const FusedConfig &cfg, const float2 *wpre, uint32_t f0, uint32_t nfr, uint32_t k0, float2 *rt);
int run64_v2_launch(const Run64v2Host &h, hipStream_t s, KernelTimer *timer);

// One call of a run kernel of the M = 1024 plan (Run1024Call, fused_common.h: one argument struct for the three kernels plus what only
// the host reads): k_run1024v2<FM, G> (kernels_run1024_v2.hip: interleaved shards, nf % 4 == 0), k_run1024v3 (kernels_run1024_v3.hip: whole
// band, one 512-thread workgroup per CU, output lines staged in registers; calls of whole 4-frame tiles) or k_shard1024<.., G>
// (kernels_shard1024.hip: chan_stride G = 4, 8, F32 or CF32 rows of the owned channels; the fold of the aliasing branches behind the FIR + a
// (1024 / G)-point DFT across the lanes of a wave).  Same state buffers and tables as k_run1024.  One launcher (kernels_run1024_v3.hip), one
// launch per call and, behind a cold one, k_run1024_dcfix; no fix-up kernel: a run computes the frame in front of it itself.
struct Run1024Call;
int run1024_launch(const Run1024Call &h, hipStream_t s, KernelTimer *timer);
// The launcher's dispatch table is filled by the kernels' own files: the instantiation for (FM, G), its workgroup size and the stamps of
// its debug trace (RUN1024_V3_TRACE_N / SHARD1024_TRACE_N; 0: not a trace build).  fn null: not built
struct Run1024Kernel { const void *fn = nullptr; unsigned threads = 0; size_t trace_n = 0; };
Run1024Kernel run1024_v2_kernel(bool fm, uint32_t G);
Run1024Kernel shard1024_kernel(bool fm, uint32_t G);
constexpr size_t RUN1024_V3_TRACE_N = 1536, SHARD1024_TRACE_N = 768;


// Single-pass DC blocker + NCO mix for whole chunks of the any-M route (kernels_dc_tile.hip), a member of GenericPlan.
// k_dc_tile looks back LOOKBACK tiles; k_dc_fold / k_dc_fold8 fold with beta^-512 ratios: a handle whose alpha does not fit them
// (dc_window_ok) has no DcTilePlan and keeps the exact block scan
bool dctile_supported(const DcParams &dc);
struct DcTilePlan {
    explicit DcTilePlan(const DcParams &dc) : dcc(true, dc) {}
    // calls of up to max_samples samples; the arrays come out of mem; cus: compute units of the handle's device (the k_dc_fold grid);
    // shard8: the handle takes mix_identity_shard (k_dc_fold8's scratch)
    int init(DeviceBuffers &mem, uint64_t max_samples, uint32_t cus, bool shard8);
    int reset(hipStream_t s);
    // pick > 0: y receives only the samples whose index in this call is a multiple of `pick` (n / pick of them)
    int process(const float2 *x, float2 *y, uint32_t n, bool do_mix, const NcoParams &nco, const float2 *nco_tab, hipStream_t s, uint32_t pick = 0);
    // DeNo --mix over all M channels, M a multiple of 4096, n a multiple of M: out[n / M] = M x (branch-0 FIR of the DC-blocked,
    // pre-mixed stream): out[t] = M sum_n taps[(M-1) + n M] u0[(p-1) + t - n]; hist_in / hist_out: the p - 1 picked samples before /
    // after the call (different buffers)
    bool mix_identity_supported(uint32_t M, uint32_t n, uint32_t taps_p) const
    {
        return M && M % 4096u == 0 && n && n % M == 0 && dcc.beta > 0.f && taps_p >= 1 && taps_p <= 33;
    }
    int mix_identity(const float2 *x, uint32_t n, const NcoParams &nco, const float2 *nco_tab, const float *taps, uint32_t M, uint32_t taps_p,
                     const float2 *hist_in, float2 *hist_out, float2 *out, hipStream_t s);
    // the same for the interleaved channel shard g of G: out[n / M] = (M / G) sum_{n2 < G} W_G^(n2 g) x (FIR of branch (M / G) n2); G <= 8,
    // (M / G) % 512 == 0; hist_in / hist_out: [G][p - 1]
    bool mix_identity_shard_supported(uint32_t M, uint32_t n, uint32_t taps_p, uint32_t G) const
    {
        return d_part8 && mix_identity_supported(M, n, taps_p) && (G == 2 || G == 4 || G == 8) && M % G == 0 && (M / G) % 512u == 0;
    }
    int mix_identity_shard(const float2 *x, uint32_t n, const NcoParams &nco, const float2 *nco_tab, const float *taps, uint32_t M, uint32_t taps_p,
                           uint32_t G, uint32_t g, const float2 *hist_in, float2 *hist_out, float2 *out, hipStream_t s);
    // sticky device-side error word (a look-back wait hit its spin limit); reads, then clears it; synchronises
    int status(unsigned *status);

    const DcConsts dcc;
    uint32_t max_nb = 0, epoch = 0, cus = 256;
    unsigned *d_ticket = nullptr, *d_status = nullptr;
    unsigned long long *d_agg = nullptr;
    float2 *d_part = nullptr;            // k_dc_fold: one aggregate and the first sample per tile
    float2 *d_part8 = nullptr;           // k_dc_fold8 (shard8): 8 aggregates + 8 first samples per tile
    float2 *d_vend[2] = {nullptr, nullptr};
    int cur = 0;
};
int  launch_branch0_fir(const float2 *u0, const float *taps, float2 *out, float2 *hist_out, uint32_t M, uint32_t p, uint32_t nf, hipStream_t s);

}  // namespace csdr
