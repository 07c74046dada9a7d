"""numpy restatement of the synthesizer of the 2x-oversampled bank of DESIGN.md 4.18 (csdr_pfbsyn2_*: the synthesizer side of
liquid's firpfbch2_crcf as recalled, which the reference does not import).  No GPU, no product code.

M channels (a power of two), semi-length m, a real prototype g[0 .. L - 1] with L = 2 m M; P = M / 2 output samples per frame of M
inputs Y[k][t], frames t counted from the start of the stream; frames t < 0 do not exist.

  truth(g, Y, M)                   (i)   the closed form in f64 as an overlap-add: frame t adds g[i] z_t[(t P + i) mod M] / 2 to
                                         sample t P + i for every i < L (P taps at a time over all frames), z_t[q] =
                                         sum_k Y_k[t] e^{+2 pi j k q / M} by a matrix product with phasors looked up by k q mod M
                                         (no parity, no history, no transform)
  structural(g, Y, M, m, prec,     (ii)  prec = 64: the recalled structure in f64, call by call.  Carried: the frame parity and the
             cuts, mutate)               last 4 m - 1 input frames (and how many of them exist).  Per frame a backward DFT
                                         (np.fft.ifft times M); output frame t reads the slots par P .. par P + P - 1, par = t mod 2,
                                         of the last 4 m transforms: x[t P + r] = 1/2 sum_n g[r + n P] w_{t-n}[par P + r]
                                   (iii) prec = 32: the same with the kernel's accumulation, acc = fma(g, w, acc) from +0 with the
                                         oldest frame first (n = 4 m - 1 down to 0), frames in front of the stream skipped (the fma
                                         as an f64 product and sum rounded to f32), and a complex64 ifft.  This is the yardstick for
                                         the GPU kernel's error, not its bit pattern
                                         cuts: frames per call (default: one call); mutate: one of MUTATIONS, a deliberate fault
                                         behind the first call boundary that the GPU bounds have to catch
  design(M, m, as_db, fc)          (iv)  pfbch2_restatement.design with the synthesizer's rule, fc = 0.5 / M when 0 is given
  roundtrip(M, m, as_db, x, ...)   (v)   the analyzer's closed form followed by (i): (rel-RMS of xh[s + D] - x[s], gain, D) behind
                                         the first L samples, D = 2 M m - M / 2 + 1
truth and structural return [frames P]."""
import numpy as np

import pfbch2_restatement as A

f32 = np.float32
MUTATIONS = ("parity", "halo")


def delay(M, m):
    return 2 * M * m - M // 2 + 1


def _rows(Y, M):
    Y = np.asarray(Y)
    assert Y.ndim == 2 and Y.shape[0] == M, (Y.shape, M)
    return Y, M // 2, Y.shape[1]


def truth(g, Y, M):
    g = np.asarray(g, np.float64).reshape(-1)
    Y, P, T = _rows(Y, M)
    L = g.size
    k = np.arange(M)
    E = np.exp(2j * np.pi * ((k[:, None] * k[None, :]) % M) / M)          # E[q][k]
    z = (E @ Y.astype(np.complex128)).T                                     # z[t][q]
    # piece n of frame t, g[n P .. n P + P - 1], lands on the samples (t + n) P + r and meets the slots ((t + n) P + r) mod M
    out = np.zeros((T + L // P, P), np.complex128)
    t, r = np.arange(T), np.arange(P)
    for n in range(L // P):
        q = (((t + n) * P) % M)[:, None] + r[None, :]
        out[n:n + T] += g[n * P:(n + 1) * P][None, :] * np.take_along_axis(z, q, axis=1)
    return 0.5 * out[:T].reshape(-1)


def structural(g, Y, M, m, prec=64, cuts=None, mutate=None):
    assert prec in (32, 64) and mutate in (None,) + MUTATIONS
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    g = np.asarray(g).reshape(-1).astype(real)
    Y, P, T = _rows(Y, M)
    assert g.size == 2 * m * M
    NT, HF = 4 * m, 4 * m - 1
    cuts = [T] if cuts is None else list(cuts)
    assert sum(cuts) == T
    hist = np.zeros((0, M), cplx)              # the input frames the stream has had, the last HF of them at most
    parity, pos, out = 0, 0, []
    r = np.arange(P)
    for call, c in enumerate(cuts):
        if mutate == "parity" and call == 1:
            parity ^= 1
        if mutate == "halo" and call == 1:
            hist = hist[1:]                    # the run's halo starts one frame late
        fr = np.concatenate([hist, np.ascontiguousarray(Y[:, pos:pos + c].T).astype(cplx)])
        seen = hist.shape[0]
        w = (np.fft.ifft(fr, axis=1) * real(M)).astype(cplx) if fr.size else fr   # numpy >= 2 transforms complex64 in f32
        i = np.arange(c)
        cols = (((parity + i) & 1) * P)[:, None] + r[None, :]
        acc_re = np.zeros((c, P), real)
        acc_im = np.zeros((c, P), real)
        for n in range(NT - 1, -1, -1):                                    # oldest frame first
            src = i - n + seen
            ok = src >= 0                                                  # frames in front of the stream are skipped
            if not ok.any():
                continue
            v = np.take_along_axis(w[src[ok]], cols[ok], axis=1)
            gn = g[r + n * P][None, :]
            if prec == 64:
                acc_re[ok] = acc_re[ok] + gn * v.real
                acc_im[ok] = acc_im[ok] + gn * v.imag
            else:
                acc_re[ok] = (gn.astype(np.float64) * v.real.astype(np.float64) + acc_re[ok].astype(np.float64)).astype(f32)
                acc_im[ok] = (gn.astype(np.float64) * v.imag.astype(np.float64) + acc_im[ok].astype(np.float64)).astype(f32)
        x = np.empty((c, P), cplx)
        x.real, x.imag = acc_re * real(0.5), acc_im * real(0.5)
        out.append(x.reshape(-1))
        hist = fr[max(0, fr.shape[0] - HF):]
        parity = (parity + c) & 1
        pos += c
    return np.concatenate(out) if out else np.zeros(0, cplx)


def yardstick(g, Y, M, m):
    return structural(g, Y, M, m, prec=32)


def design(M, m, as_db, fc=0.0):
    return A.design(M, m, as_db, 0.5 / M if fc == 0 else fc)


def by_phase(x, M):
    """[frames P] -> [P][frames]: one row per output phase r, so that the per-row rule of pfbch2_restatement.ratios sees a
    single wrong branch undiluted"""
    return np.ascontiguousarray(np.asarray(x).reshape(-1, M // 2).T)


def roundtrip(M, m, as_db, x, fc_a=0.0, fc_s=0.0):
    """analysis with the prototype cut at fc_a (0: 1 / M), synthesis with the one cut at fc_s (0: 0.5 / M), both in f64;
    returns (rms(xh[s + D] - x[s]) / rms(x[s]), |<x, xh>| / <x, x>, D) over L <= s < n - D"""
    L, D = 2 * M * m, delay(M, m)
    x = np.asarray(x, np.complex128).reshape(-1)
    Y = A.truth(A.design(M, m, as_db, fc_a)[:L], x, M)
    xh = truth(design(M, m, as_db, fc_s)[:L], Y, M)
    a, b = x[L:x.size - D], xh[L + D:]
    assert a.size == b.size and a.size > 0
    rel = float(np.sqrt(np.mean(np.abs(b - a) ** 2) / np.mean(np.abs(a) ** 2)))
    gain = float(np.abs(np.vdot(a, b)) / np.vdot(a, a).real)
    return rel, gain, D
