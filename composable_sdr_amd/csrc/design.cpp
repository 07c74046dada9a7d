// Host-side filter / oscillator design for libcsdr_hip.so (product code).
// Mirrors what the reference obtains from liquid-dsp at object creation:
//   firpfbch_crcf_create_kaiser(0, M, 7, 80.0)            Liquid.chs:813
//   nco_crcf_create(LIQUID_VCO) + set_frequency(offset)    Liquid.chs:816-818
//   agc_crcf_squelch_set_threshold                         Liquid.chs:713
#include "../../include/csdr.h"
#include "csdr_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <utility>

namespace csdr {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char *last_error() { return g_err; }

int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
    set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    return e == hipErrorOutOfMemory ? -5 : -2;
}

// Modified Bessel function I0 by its power series (converged to f64 precision).
static double bessel_i0(double z)
{
    double q = 0.25 * z * z, term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

static double kaiser_beta(double As)
{
    As = std::fabs(As);
    if (As > 50.0) return 0.1102 * (As - 8.7);
    if (As > 21.0) return 0.5842 * std::pow(As - 21.0, 0.4) + 0.07886 * (As - 21.0);
    return 0.0;
}

std::vector<float> design_pfb_taps(uint32_t M, uint32_t m, float As)
{
    const uint32_t N = 2 * M * m + 1;          // designed length; the bank uses N-1 taps
    const double fc = 0.5 / (double)M;
    const double beta = kaiser_beta(As), ib = bessel_i0(beta);
    const double pi = 3.14159265358979323846;
    std::vector<float> h((size_t)M * 2 * m);
    for (uint32_t i = 0; i < N - 1; i++) {
        double t = (double)i - 0.5 * (double)(N - 1);
        double x = 2.0 * fc * t;
        // liquid's sincf uses a cosine product below |x| < 0.01 (exact to ~1e-10 there)
        double sinc = std::fabs(x) < 0.01
                          ? std::cos(pi * x / 2) * std::cos(pi * x / 4) * std::cos(pi * x / 8)
                          : std::sin(pi * x) / (pi * x);
        double r = 2.0 * t / (double)(N - 1);
        double a = 1.0 - r * r;
        double w = bessel_i0(beta * std::sqrt(a > 0 ? a : 0)) / ib;
        h[i] = (float)(sinc * w);
    }
    return h;
}

// liquid_firdes_kaiser(N, fc, As, 0): h[i] = sinc(2 fc t) w_kaiser(i), t = i - (N-1)/2 (f64).  The window's argument is
// 2 t / wden, wden = N - 1 (what KAT1 pins) unless the caller passes another; dt is liquid's fractional sample offset mu, added to t
static std::vector<double> firdes_kaiser(uint32_t N, double fc, double As, double wden = 0.0, double dt = 0.0)
{
    if (wden == 0.0) wden = (double)(N - 1);
    const double beta = kaiser_beta(As), ib = bessel_i0(beta);
    const double pi = 3.14159265358979323846;
    std::vector<double> h(N);
    for (uint32_t i = 0; i < N; i++) {
        double t = (double)i - 0.5 * (double)(N - 1) + dt;
        double x = 2.0 * fc * t;
        double sinc = std::fabs(x) < 0.01
                          ? std::cos(pi * x / 2) * std::cos(pi * x / 4) * std::cos(pi * x / 8)
                          : std::sin(pi * x) / (pi * x);
        double r = 2.0 * t / wden;
        double a = 1.0 - r * r;
        h[i] = sinc * bessel_i0(beta * std::sqrt(a > 0 ? a : 0)) / ib;
    }
    return h;
}

// ---- firpfbch2_crcf_create_kaiser(ANALYZER, M, m, As) as recalled (unpinned) ----
// liquid_firdes_kaiser(2 M m + 1, fc, As, 0) with fc = 1 / M for an analyzer ("twice the synthesizer's bandwidth"), scaled so that
// the taps sum to M; f64, rounded once
std::vector<float> design_pfb2_taps(uint32_t M, uint32_t m, float As, float fc)
{
    const uint32_t N = 2 * M * m + 1;
    const std::vector<double> hd = firdes_kaiser(N, fc == 0.f ? 1.0 / (double)M : (double)fc, (double)As);
    double sum = 0.0;
    for (double v : hd) sum += v;
    std::vector<float> h(N);
    for (uint32_t i = 0; i < N; i++) h[i] = (float)(hd[i] * (double)M / sum);
    return h;
}

// ---- multi-stage resampler (msresamp_crcf's structure; "csdr msresamp v1" parameters) ----
ResampDesign design_msresamp(float rate, float As)
{
    ResampDesign d;
    d.rate = rate; d.rho = (double)rate; d.K = 0;
    while (d.rho < 0.5 && d.K < 24) { d.K++; d.rho *= 2.0; }
    for (uint32_t s = 0; s < d.K; s++) {
        // half-band stage s sees the final band at fb = 0.45 r 2^s of its input rate
        double fb = 0.45 * (double)rate * (double)(1u << s), ft = 0.5 - 2.0 * fb;
        if (ft < 0.01) ft = 0.01;
        double N = (std::fabs((double)As) - 7.95) / (14.36 * ft);
        int m = (int)std::ceil((N - 1.0) / 4.0);
        if (m < 2) m = 2;
        std::vector<double> hd = firdes_kaiser(4 * m + 1, 0.25, As);
        std::vector<float> h(4 * m + 1);
        for (size_t i = 0; i < h.size(); i++) h[i] = (float)(0.5 * hd[i]);
        d.m_hb.push_back((uint32_t)m); d.h_hb.push_back(h);
    }
    d.npfb = 256; d.m_arb = 7;
    double fc = 0.515 * d.rho; if (fc > 0.49) fc = 0.49;
    d.fc = (float)fc;
    const uint32_t P = 2 * d.m_arb;
    std::vector<double> hd = firdes_kaiser(P * d.npfb + 1, fc / (double)d.npfb, As);
    d.pfb.resize((size_t)d.npfb * P);
    for (uint32_t b = 0; b < d.npfb; b++)
        for (uint32_t j = 0; j < P; j++) d.pfb[(size_t)b * P + j] = (float)(2.0 * fc * hd[b + (size_t)j * d.npfb]);
    d.delta = (uint64_t)std::llround(4294967296.0 / d.rho);
    return d;
}

// ---- rowResampler ("csdr rowresamp v1"): the arbitrary stage above on its own, with m and the stretch D free ----
bool rowresamp_design_args_ok(double rate, uint32_t m, float as_db, float fc)
{
    if (!(rate >= 0.125 && rate <= 8.0) || !(as_db > 0.f && as_db <= 120.f) || !(fc >= 0.f && fc < 0.5f)) return false;
    return rrs_args_ok((uint64_t)std::llround(4294967296.0 / rate), m);
}
RowResampDesign design_rowresamp(double rate, uint32_t m, float as_db, float fc_)
{
    RowResampDesign d;
    d.delta = (uint64_t)std::llround(4294967296.0 / rate);
    d.P = rrs_P(d.delta, m);
    double fc = (double)fc_;
    if (fc_ == 0.f) { fc = 0.515 * (rate < 1.0 ? rate : 1.0); if (fc > 0.49) fc = 0.49; }
    d.fc = (float)fc;
    const std::vector<double> g = firdes_kaiser(d.P * RRS_NPFB + 1, fc / (double)RRS_NPFB, (double)as_db);
    d.bank.resize((size_t)(RRS_NPFB + 1) * d.P);
    for (uint32_t b = 0; b <= RRS_NPFB; b++)
        for (uint32_t j = 0; j < d.P; j++) d.bank[(size_t)b * d.P + j] = (float)(2.0 * fc * g[b + (size_t)j * RRS_NPFB]);
    return d;
}

// 2nd-order Butterworth low-pass by the bilinear transform with pre-warping (liquid iirdes BUTTER/LOWPASS/SOS, order 2)
BiquadParams design_butter2_lowpass(float fc)
{
    BiquadParams p{};
    const double K = std::tan(3.14159265358979323846 * (double)fc), n = 1.0 / (1.0 + std::sqrt(2.0) * K + K * K);
    p.b0 = (float)(K * K * n); p.b1 = (float)(2.0 * K * K * n); p.b2 = p.b0;
    p.a1 = (float)(2.0 * (K * K - 1.0) * n); p.a2 = (float)((1.0 - std::sqrt(2.0) * K + K * K) * n);
    // powers of the state matrix of the f32 coefficients: A^(16), A^(32), ... A^(2048)
    double A[4] = {-(double)p.a1, -(double)p.a2, 1.0, 0.0};
    auto mul = [](const double *x, const double *y, double *z) {
        double t[4] = {x[0] * y[0] + x[1] * y[2], x[0] * y[1] + x[1] * y[3], x[2] * y[0] + x[3] * y[2], x[2] * y[1] + x[3] * y[3]};
        for (int i = 0; i < 4; i++) z[i] = t[i];
    };
    double P[4] = {A[0], A[1], A[2], A[3]};
    for (int i = 0; i < 4; i++) mul(P, P, P);                    // A^16
    for (int k = 0; k < 8; k++) {
        for (int i = 0; i < 4; i++) p.pw[k][i] = P[i];
        mul(P, P, P);
    }
    return p;
}

std::vector<float> design_firdecim_kaiser(uint32_t M, uint32_t m, float As)
{
    const uint32_t N = 2 * M * m + 1;
    std::vector<double> hd = firdes_kaiser(N, 0.5 / (double)M, As);
    std::vector<float> h(N);
    for (uint32_t i = 0; i < N; i++) h[i] = (float)hd[i];
    return h;
}

// ---- stereoFMDecoder' quadRate decim (Liquid.chs:985-1078), DESIGN.md 4.9 ----
// fir_group_delay(h, n, fc) = Re(sum i h[i] e^{j 2 pi fc i} / sum h[i] e^{j 2 pi fc i}), accumulated in f32 (liquid-dsp 1.3.2 as
// recalled; the complex quotient's real part is taken as (t0 conj(t1)).re / |t1|^2 in f32)
float fir_group_delay(const std::vector<float> &h, float fc)
{
    float t0r = 0.f, t0i = 0.f, t1r = 0.f, t1i = 0.f;
    for (size_t i = 0; i < h.size(); i++) {
        const float a = (float)(2.0 * 3.14159265358979323846 * (double)fc * (double)i);
        const float c = cosf(a), s = sinf(a), hc = h[i] * c, hs = h[i] * s, fi = (float)i;
        t0r = t0r + hc * fi; t0i = t0i + hs * fi;
        t1r = t1r + hc; t1i = t1i + hs;
    }
    const float num = t0r * t1r + t0i * t1i, den = t1r * t1r + t1i * t1i;
    return num / den;
}

FmsDesign design_fmstereo(double quad_rate, uint32_t decim)
{
    FmsDesign f;
    const double pi = 3.14159265358979323846;
    f.N = (uint32_t)std::nearbyint(quad_rate / 1350.0);                  // Haskell `round` (half-even) of quadRate / 1350
    const float fc_pilot = (float)(800.0 / quad_rate), fc_audio = (float)(15000.0 / quad_rate);
    std::vector<double> hp = firdes_kaiser(f.N, (double)fc_pilot, 60.0), ha = firdes_kaiser(f.N, (double)fc_audio, 60.0);
    f.h_pilot.resize(f.N); f.h_audio.resize(f.N);
    for (uint32_t i = 0; i < f.N; i++) { f.h_pilot[i] = (float)hp[i]; f.h_audio[i] = (float)ha[i]; }
    f.scale_pilot = 2.0f * fc_pilot; f.scale_audio = 2.0f * fc_audio;   // firfiltCreateCKaiser: set_scale (2 fc)
    f.d = (uint32_t)std::nearbyint(fir_group_delay(f.h_pilot, (float)(100.0 / quad_rate)));
    const float ncoF = (float)(19000.0 * 2.0 * pi / quad_rate);
    f.d_nco = nco_freq_word(ncoF);
    f.alpha = (float)(9.0 / quad_rate);                                   // nco_crcf_pll_set_bandwidth: alpha = bw, beta = sqrtf(alpha)
    f.beta = sqrtf(f.alpha);
    f.bq = design_butter2_lowpass((float)(5000.0 / quad_rate));
    f.h_dec = design_firdecim_kaiser(decim, 10, 60.0f);
    return f;
}

// ---- firhilbf_create(m, As) (Liquid.chs:503-546), DESIGN.md 4.11 ----
// h = liquid_firdes_kaiser(4 m + 1, 0.25, As, 0); hc[i] = h[i] e^{j pi t / 2}, t = i - 2 m; hq[j] = Im hc[4 m - i], i = 2 j + 1.
// t is odd there, so the factor is exactly +-1: the prototype in f64, rounded once.  The Kaiser window's argument is 2 t / h_len
// here, not the 2 t / (h_len - 1) of the other designs: that is what the tap table this block was specified by holds
// (0.0065559 .. 0.6219635 for m = 5, As = 60), and nothing pins liquid's firhilbf taps either way.
std::vector<float> design_firhilb(uint32_t m, float As)
{
    const uint32_t h_len = 4 * m + 1;
    const std::vector<double> h = firdes_kaiser(h_len, 0.25, As, (double)h_len);
    std::vector<float> hq(2 * m);
    for (uint32_t j = 0; j < 2 * m; j++) {
        const uint32_t i = h_len - (2 * j + 1) - 1;
        const int t = (int)i - (int)(2 * m);
        hq[j] = (float)((((t % 4) + 4) % 4 == 1) ? h[i] : -h[i]);
    }
    return hq;
}

// symsync_create(k, M, H, H_len)'s part behind the prototype d.H (H_len = 2 M k m + 1 taps, f32): the derivative with the
// wrap-around ends, its 0.06 / max |H dH| scale and the two reversed tap-major banks, all in f32 as liquid does
void symsync_set_prototype(SymsyncDesign &d)
{
    const uint32_t N = d.H_len, M = d.M;
    d.dH.resize(N);
    float hdh_max = 0.f;
    for (uint32_t i = 0; i < N; i++) {
        d.dH[i] = i == 0 ? d.H[1] - d.H[N - 1] : (i == N - 1 ? d.H[0] - d.H[i - 1] : d.H[i + 1] - d.H[i - 1]);
        const float p = d.H[i] * d.dH[i];
        if (std::fabs(p) > hdh_max || i == 0) hdh_max = std::fabs(p);
    }
    const float s = 0.06f / hdh_max;
    for (uint32_t i = 0; i < N; i++) d.dH[i] = d.dH[i] * s;
    d.mf.resize((size_t)d.L * M); d.dmf.resize((size_t)d.L * M);
    for (uint32_t j = 0; j < d.L; j++)
        for (uint32_t p = 0; p < M; p++) {
            d.mf[(size_t)j * M + p] = d.H[p + (d.L - 1 - j) * M];          // loaded reversed: the newest sample meets H[p]
            d.dmf[(size_t)j * M + p] = d.dH[p + (d.L - 1 - j) * M];
        }
}

// ---- symsync_rrrf_create_kaiser(k, m, beta, M) + set_lf_bw + set_output_rate (Liquid.chs:244-282), DESIGN.md 4.10 ----
// liquid-dsp 1.3.2 as recalled (unpinned): H_len = 2 M k m + 1, Hf = liquid_firdes_kaiser(H_len, 0.75f / (k M), 40, 0) in f64,
// H = Hf 2 0.75 rounded once to f32 (beta is ignored); the derivative, its scale and the loop filter in f32 as liquid does.
SymsyncDesign design_symsync_kaiser(uint32_t k, uint32_t m, float beta, uint32_t M, float lf_bw, uint32_t k_out)
{
    (void)beta;
    SymsyncDesign d;
    d.k = k; d.m = m; d.M = M; d.k_out = k_out;
    d.H_len = 2 * M * k * m + 1;
    d.L = d.H_len / M;                                                   // firpfb: integer division drops the last tap
    const float fc = 0.75f / (float)(k * M);
    std::vector<double> hd = firdes_kaiser(d.H_len, (double)fc, 40.0);
    const uint32_t N = d.H_len;
    d.H.resize(N);
    for (uint32_t i = 0; i < N; i++) d.H[i] = (float)(hd[i] * 1.5);
    symsync_set_prototype(d);
    // set_lf_bw(bt): B = {0.22 bt, 0, 0}, A = {1 - 0.5 (1 - bt), -0.495 (1 - bt), 0}; iirfiltsos divides both by A[0]
    const float alpha = 1.0f - lf_bw, lb = 0.22f * lf_bw, ha = 0.5f * alpha, hb = 0.495f * alpha;
    const float A0 = 1.0f - ha, A1 = -hb, A2 = 0.0f;
    d.b0 = lb / A0; d.b1 = 0.0f / A0; d.b2 = 0.0f / A0; d.a1 = A1 / A0; d.a2 = A2 / A0;
    d.rate_adj = (float)(0.5 * (double)lf_bw);
    d.init = SymsyncState{};
    d.init.rate = (float)k / (float)k_out;                               // set_output_rate: rate = del = k / k_out
    d.init.del = d.init.rate;
    return d;
}

// ---- liquid_firdes_prototype(ARKAISER | RRC, k, m, beta, dt) (symSyncC, Liquid.chs:177-242), csdr_firdes_rnyquist; DESIGN.md 4.16 ----
// n = 2 k m + 1 taps in f64.  RRC is liquid_firdes_rrcos' closed form.  ARKAISER is liquid_firdes_arkaiser as recalled: the
// r-Kaiser filter with the approximation rho_hat of the bandwidth factor that minimises the inter-symbol interference of h * h
// (the property tests/test_rnyquist_cpu.py pins); As comes from Kaiser's length formula, where liquid bisects an estimate
// (deviation).  An empty vector: rho_hat outside (0, 1), where liquid switches to a second approximation not reproduced here.
static std::vector<double> design_rnyquist_f64(int ftype, uint32_t k, uint32_t m, double beta, double dt)
{
    const double pi = 3.14159265358979323846;
    const uint32_t n = 2 * k * m + 1;
    std::vector<double> h(n);
    if (ftype == CSDR_FIRFILT_RRC) {
        for (uint32_t i = 0; i < n; i++) {
            const double z = ((double)i + dt) / (double)k - (double)m;
            const double g = 1.0 - 16.0 * beta * beta * z * z;
            if (std::fabs(z) < 1e-12) h[i] = 1.0 - beta + 4.0 * beta / pi;
            else if (std::fabs(g) < 1e-8)
                h[i] = beta / std::sqrt(2.0) * ((1.0 + 2.0 / pi) * std::sin(pi / (4.0 * beta)) + (1.0 - 2.0 / pi) * std::cos(pi / (4.0 * beta)));
            else h[i] = (std::sin(pi * z * (1.0 - beta)) + 4.0 * beta * z * std::cos(pi * z * (1.0 + beta))) / (pi * z * g);
        }
        return h;
    }
    const double lb = std::log(beta), lm = std::log((double)m);
    const double c0 = 0.762886 + 0.067663 * lm, c1 = 0.065515, c2 = std::log(1.0 - 0.088 * std::pow((double)m, -1.6));
    const double rho_hat = c0 + c1 * lb + c2 * lb * lb;
    if (!(rho_hat > 0.0 && rho_hat < 1.0)) return {};
    const double kf = 0.5 * (1.0 + beta * (1.0 - rho_hat)) / (double)k, del = beta * rho_hat / (double)k;
    const double As = 14.26 * del * (double)n + 7.95;
    h = firdes_kaiser(n, kf, As, 0.0, dt);
    double e2 = 0.0;
    for (double v : h) e2 += v * v;
    const double g = std::sqrt((double)k / e2);
    for (double &v : h) v *= g;
    return h;
}

std::vector<float> design_rnyquist(int ftype, uint32_t k, uint32_t m, float beta, float dt)
{
    const std::vector<double> h = design_rnyquist_f64(ftype, k, m, (double)beta, (double)dt);
    return std::vector<float>(h.begin(), h.end());
}

// ---- fskdem_create(m, k, bandwidth) (Liquid.chs:336-382), DESIGN.md 4.12 ----
// liquid-dsp 1.3.2 as recalled (unpinned), all of it in f32 as liquid does it: the transform size K is the K_hat in
// [k, max(16, 4 k)] whose tone spacing 0.5 df K_hat lies nearest an integer (the first of equals; the search stops at the
// first error below 1e-6), and tone i sits in bin roundf(freq K), a negative one wrapped by + K.  A wrapped index that rounds
// to K itself (a tone less than half a bin below 0) names bin 0; liquid would read one past its buffer there.
FskdemDesign design_fskdem(uint32_t m, uint32_t k, float bandwidth)
{
    FskdemDesign d;
    d.m = m; d.k = k; d.M = 1u << m;
    const float M2 = 0.5f * (float)(d.M - 1);
    const float df = bandwidth / M2;
    const uint32_t K_min = k, K_max = 4 * k > 16 ? 4 * k : 16;
    float err_min = 0.f;
    d.K = K_min;
    for (uint32_t K_hat = K_min; K_hat <= K_max; K_hat++) {
        const float v = 0.5f * df * (float)K_hat;
        const float err = std::fabs(roundf(v) - v);
        if (K_hat == K_min || err < err_min) { d.K = K_hat; err_min = err; }
        if (err < 1e-6f) break;
    }
    d.map.resize(d.M);
    for (uint32_t i = 0; i < d.M; i++) {
        const float freq = ((float)i - M2) * bandwidth / M2;
        const float idx = freq * (float)d.K;
        d.map[i] = (uint32_t)roundf(idx < 0.f ? idx + (float)d.K : idx) % d.K;
    }
    for (uint32_t i = 0; i < d.M && !d.repeated; i++)
        for (uint32_t j = 0; j < i; j++) if (d.map[i] == d.map[j]) { d.repeated = true; break; }
    // W[t] = e^{-2 pi i t / K}: evaluated in f64, rounded once
    d.W.resize(2 * (size_t)d.K);
    for (uint32_t t = 0; t < d.K; t++) {
        const double a = 2.0 * 3.14159265358979323846 * (double)t / (double)d.K;
        d.W[2 * t] = (float)std::cos(a);
        d.W[2 * t + 1] = (float)-std::sin(a);
    }
    return d;
}

// ---- firfiltCreateCKaiser n fc as mu (Liquid.chs:889-895), csdr_firdes_kaiser; DESIGN.md 4.13 ----
std::vector<float> design_firfilt_kaiser(uint32_t n, float fc, float As)
{
    const std::vector<double> hd = firdes_kaiser(n, (double)fc, (double)As);
    std::vector<float> h(n);
    for (uint32_t i = 0; i < n; i++) h[i] = (float)hd[i];
    return h;
}

// ---- gmskdem_create(k, m, BT) (Liquid.chs:384-429) and firfilt_rrrf_create_rnyquist(GMSKRX, ..) (:935-953), csdr_firdes_gmsktx /
// csdr_firdes_gmskrx; DESIGN.md 4.15 ----
// The transmit pulse is the textbook one: a rectangle of one symbol through a Gaussian of bandwidth-time product BT, sampled at
// t_i = i / k - m: g~_i = Q(c (t_i - 1/2)) - Q(c (t_i + 1/2)), c = 2 pi BT / sqrt(ln 2), Q(x) = erfc(x / sqrt 2) / 2, scaled to
// sum one (liquid scales to pi / 2 k: that factor is the modulator's business here).
static std::vector<double> design_gmsktx_f64(uint32_t k, uint32_t m, double bt)
{
    const uint32_t L = 2 * k * m + 1;
    const double c = 2.0 * 3.14159265358979323846 * bt / std::sqrt(std::log(2.0));
    auto Q = [](double x) { return 0.5 * std::erfc(x / std::sqrt(2.0)); };
    std::vector<double> g(L);
    double sum = 0.0;
    for (uint32_t i = 0; i < L; i++) {
        const double t = (double)i / (double)k - (double)m;
        g[i] = Q(c * (t - 0.5)) - Q(c * (t + 0.5));
        sum += g[i];
    }
    for (double &v : g) v /= sum;
    return g;
}

std::vector<float> design_gmsktx(uint32_t k, uint32_t m, float bt)
{
    const std::vector<double> g = design_gmsktx_f64(k, m, (double)bt);
    return std::vector<float>(g.begin(), g.end());
}

// The receive filter is this library's own, not liquid_firdes_gmskrx (whose construction is not pinned): with c = g * r (full
// convolution, centre L - 1) it asks c[L - 1] = 1 and c[L - 1 + j k] = 0 for 0 < |j| <= m, which is A r = e_m with
// A[j + m][i] = g[L - 1 + j k - i], and takes the solution of least sum r^2 (least noise gain): r = A^T lambda,
// (A A^T) lambda = e_m.  The system has order 2 m + 1 <= 17 and a condition number of at most 61 (BT = 0.2): Gaussian
// elimination with partial pivoting in f64.  r is made symmetric before it is rounded, so the f32 taps are exactly symmetric.
std::vector<float> design_gmskrx(uint32_t k, uint32_t m, float bt)
{
    const std::vector<double> g = design_gmsktx_f64(k, m, (double)bt);
    const int L = (int)g.size(), R = 2 * (int)m + 1;
    std::vector<double> A((size_t)R * L, 0.0);
    for (int j = 0; j < R; j++)
        for (int i = 0; i < L; i++) {
            const int idx = L - 1 + (j - (int)m) * (int)k - i;
            if (idx >= 0 && idx < L) A[(size_t)j * L + i] = g[idx];
        }
    std::vector<double> N((size_t)R * R), lam(R, 0.0);
    for (int a = 0; a < R; a++)
        for (int b = 0; b < R; b++) {
            double s = 0.0;
            for (int i = 0; i < L; i++) s += A[(size_t)a * L + i] * A[(size_t)b * L + i];
            N[(size_t)a * R + b] = s;
        }
    lam[m] = 1.0;
    for (int p = 0; p < R; p++) {
        int best = p;
        for (int a = p + 1; a < R; a++) if (std::fabs(N[(size_t)a * R + p]) > std::fabs(N[(size_t)best * R + p])) best = a;
        if (best != p) {
            for (int b = 0; b < R; b++) std::swap(N[(size_t)p * R + b], N[(size_t)best * R + b]);
            std::swap(lam[p], lam[best]);
        }
        for (int a = p + 1; a < R; a++) {
            const double f = N[(size_t)a * R + p] / N[(size_t)p * R + p];
            for (int b = p; b < R; b++) N[(size_t)a * R + b] -= f * N[(size_t)p * R + b];
            lam[a] -= f * lam[p];
        }
    }
    for (int p = R - 1; p >= 0; p--) {
        double s = lam[p];
        for (int b = p + 1; b < R; b++) s -= N[(size_t)p * R + b] * lam[b];
        lam[p] = s / N[(size_t)p * R + p];
    }
    std::vector<double> r(L, 0.0);
    for (int i = 0; i < L; i++)
        for (int j = 0; j < R; j++) r[i] += A[(size_t)j * L + i] * lam[j];
    std::vector<float> h(L);
    for (int i = 0; i < L; i++) h[i] = (float)(0.5 * (r[i] + r[L - 1 - i]));
    return h;
}

// ---- iirCFilter n fc f0 ap as (Liquid.chs:594-608), csdr_iirdes_butter_lowpass; DESIGN.md 4.14 ----
// Analog prototype poles exp(+-j theta_i), theta_i = (2 (i + 1) + n - 1) pi / (2 n), and -1 for odd n; p_d = (1 + m p) / (1 - m p)
// with m = tan(pi fc); all zeros at -1.  A pair gives A = [1, -2 Re p_d, |p_d|^2], B = g [1, 2, 1]; the real pole A = [1, -p_d, 0],
// B = g [1, 1, 0].  g makes the section's DC gain one: (1 + a1 + a2) / 4 = |1 - p_d|^2 / 4 = m^2 / |1 - m p|^2 for a pair and
// (1 - p_d) / 2 = m / (1 + m) for the real pole, taken in the forms that do not cancel
void design_butter_lowpass_sos(uint32_t n, float fc, float *b, float *a)
{
    const double pi = 3.14159265358979323846, m = std::tan(pi * (double)fc);
    const uint32_t L = n / 2;
    for (uint32_t i = 0; i < L; i++) {
        const double theta = (double)(2 * (i + 1) + n - 1) * pi / (double)(2 * n);
        const double pr = std::cos(theta), pim = std::sin(theta);
        const double dr = 1.0 - m * pr, di = -m * pim, den = dr * dr + di * di;                 // |1 - m p|^2
        const double nr = 1.0 + m * pr, ni = m * pim;
        const double re = (nr * dr + ni * di) / den, mag2 = (nr * nr + ni * ni) / den, g = m * m / den;
        a[3 * i] = 1.f; a[3 * i + 1] = (float)(-2.0 * re); a[3 * i + 2] = (float)mag2;
        b[3 * i] = (float)g; b[3 * i + 1] = (float)(2.0 * g); b[3 * i + 2] = (float)g;
    }
    if (n & 1) {
        const double pd = (1.0 - m) / (1.0 + m), g = m / (1.0 + m);
        a[3 * L] = 1.f; a[3 * L + 1] = (float)(-pd); a[3 * L + 2] = 0.f;
        b[3 * L] = (float)g; b[3 * L + 1] = (float)g; b[3 * L + 2] = 0.f;
    }
}

IirSosSection make_iirsos_section(const float *b, float a1, float a2)
{
    IirSosSection q{};
    q.b0 = b[0]; q.a1 = a1; q.a2 = a2;
    q.k1 = (float)((double)b[1] - (double)b[0] * (double)a1);
    q.k2 = (float)((double)b[2] - (double)b[0] * (double)a2);
    // powers of the state matrix of the f32 coefficients: A^(16), A^(32), ... A^(2048), as design_butter2_lowpass has them
    auto mul = [](const double *x, const double *y, double *z) {
        double t[4] = {x[0] * y[0] + x[1] * y[2], x[0] * y[1] + x[1] * y[3], x[2] * y[0] + x[3] * y[2], x[2] * y[1] + x[3] * y[3]};
        for (int i = 0; i < 4; i++) z[i] = t[i];
    };
    double P[4] = {-(double)a1, -(double)a2, 1.0, 0.0};
    for (int i = 0; i < 4; i++) mul(P, P, P);
    for (int k = 0; k < 8; k++) {
        for (int i = 0; i < 4; i++) q.pw[k][i] = P[i];
        mul(P, P, P);
    }
    return q;
}

uint32_t nco_freq_word(float freq)
{
    float p = (float)((double)freq * 0.159154943091895);   // freq / 2pi, rounded to f32
    float fpart = p - (float)((long)p);
    if (fpart < 0.0f) fpart += 1.0f;
    return (uint32_t)(fpart * (float)0xffffffffu);
}

float pfb_premix_freq(uint32_t M)
{
    // evaluated left to right in binary32 like the Haskell expression
    float n = (float)M;
    float a = -0.5f * (n - 1.0f);
    a = a / n;
    a = a * 2.0f;
    a = a * (float)3.14159265358979323846;
    return a;
}

void nco_phasor(uint32_t theta, float *c, float *s)
{
    // nco_crcf_get_phase(): 2*pi*theta/2^32 with theta converted to f32 first
    float ph = (float)(2.0 * 3.14159265358979323846 * (double)(float)theta / 4294967296.0);
    *c = cosf(ph);
    *s = sinf(ph);
}

uint32_t nco_period(uint32_t d_theta, uint32_t limit)
{
    if (d_theta == 0) return 1;
    // period = 2^32 / gcd(d_theta, 2^32) = 2^(32 - ctz(d_theta))
    int tz = __builtin_ctz(d_theta);
    uint64_t per = 1ull << (32 - tz);
    return per <= limit ? (uint32_t)per : 0;
}

float agc_gain_threshold(float thr_db)
{
    // rssi(g) = (float)(-20*log10((double)g)) is non-increasing in g.  Find the smallest
    // positive f32 g with rssi(g) <= thr by bisection on the f32 bit pattern.
    auto exceeded = [&](float g) { return (float)(-20.0 * std::log10((double)g)) > thr_db; };
    uint32_t lo = 0x00800000u;     // smallest normal: rssi ~ +758 dB -> exceeded
    uint32_t hi = 0x7f7fffffu;     // FLT_MAX: rssi ~ -770 dB
    float flo, fhi;
    memcpy(&flo, &lo, 4); memcpy(&fhi, &hi, 4);
    if (!exceeded(flo)) return 0.0f;                 // never exceeded
    if (exceeded(fhi)) return INFINITY;              // always exceeded
    while (hi - lo > 1) {
        uint32_t mid = lo + (hi - lo) / 2;
        float fm; memcpy(&fm, &mid, 4);
        if (exceeded(fm)) lo = mid; else hi = mid;
    }
    memcpy(&fhi, &hi, 4);
    return fhi;
}

}  // namespace csdr
