"""numpy restatement of the row resampler ("csdr rowresamp v1", csdr_rowresamp_*).  No GPU, no oracle.

  delta_of(rate), D_of(delta), P_of(delta, m), fc_of(rate, fc)    the integers and the cutoff of the spec
  design(rate, m, as_db, fc)     (bank f64 [257][P], delta): the design in f64, to be rounded once to f32
  count(T, delta, n), step(T, delta, n)   the integer timing of a call: its output count, and (count, the next call's T)
  times(T, delta, n_out)         (n_k, b, mu) of a call's outputs, exact
  truth(bank, delta, x)          (y, A) in f64 from the handle's own f32 bank, one gather of [n_out][P] indices per row:
                                 y_k = (1 - mu) s0 + mu s1 and the bound's A_k = (1 - mu) sum_j |bank[b][j] x[n_k - j]| + mu sum_j
                                 |bank[b + 1][j] x[n_k - j]| per component (re + j im for complex rows)
  yardstick(bank, delta, x)      the kernel's arithmetic in f32: P fmas per sum in the order j = 0 .. P - 1, one product, one fma
  bound(A, P)                    (P + 3) 2^-24 A_k: P fmas in any order, one product and one fma
  fskmod(sym, sps, bw_in)        2-FSK with a fractional number of samples per symbol, phase-continuous

x is [n] or [rows][n], F32 or CF32; the whole stream in one call from T = 0, x[s < 0] = 0."""
import numpy as np

from symsyncc_restatement import kaiser_f64

f32 = np.float32
U = 2.0 ** -24
NPFB = 256
ONE = 1 << 32


def delta_of(rate):
    """llround(2^32 / rate): Q32.32 input samples per output (half away from zero; the quotient is positive)"""
    return int(np.floor(4294967296.0 / float(rate) + 0.5))


def D_of(delta):
    return 1 if delta <= ONE else (delta + ONE - 1) >> 32


def P_of(delta, m):
    return 2 * m * D_of(delta)


def fc_of(rate, fc=0.0):
    return min(0.515 * min(float(rate), 1.0), 0.49) if fc == 0 else float(fc)


def design(rate, m, as_db, fc=0.0):
    delta = delta_of(rate)
    P = P_of(delta, m)
    fc = fc_of(rate, fc)
    g = kaiser_f64(P * NPFB + 1, fc / NPFB, as_db)
    idx = np.arange(NPFB + 1)[:, None] + NPFB * np.arange(P)[None, :]
    return 2.0 * fc * g[idx], delta


def count(T, delta, n):
    return 0 if (T >> 32) >= n else ((n << 32) - 1 - T) // delta + 1


def step(T, delta, n):
    c = count(T, delta, n)
    return c, T + c * delta - (n << 32)


def times(T, delta, n_out):
    t = np.uint64(T) + np.arange(n_out, dtype=np.uint64) * np.uint64(delta)
    nk = (t >> np.uint64(32)).astype(np.int64)
    b = ((t >> np.uint64(24)) & np.uint64(255)).astype(np.int64)
    mu = (t & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return nk, b, mu


def _rows(x):
    x = np.asarray(x)
    return (x.reshape(1, -1) if x.ndim == 1 else x), x.ndim == 1


def _gather(row, nk, P):
    """[n_out][P]: x[n_k - j] with zeros in front of the stream"""
    pad = np.concatenate([np.zeros(P - 1, row.dtype), row])
    return pad[(nk[:, None] + (P - 1)) - np.arange(P)[None, :]]


def truth(bank, delta, x):
    rows, one = _rows(x)
    cplx = np.iscomplexobj(rows)
    bank = np.asarray(bank, np.float64)
    P = bank.shape[1]
    n_out = count(0, delta, rows.shape[1])
    nk, b, mu = times(0, delta, n_out)
    b0, b1 = bank[b], bank[b + 1]
    Y = np.empty((rows.shape[0], n_out), np.complex128 if cplx else np.float64)
    A = np.empty_like(Y)
    for r in range(rows.shape[0]):
        xg = _gather(rows[r].astype(np.complex128 if cplx else np.float64), nk, P)
        Y[r] = (1.0 - mu) * (b0 * xg).sum(axis=1) + mu * (b1 * xg).sum(axis=1)
        if cplx:
            ar = (1.0 - mu) * np.abs(b0 * xg.real).sum(axis=1) + mu * np.abs(b1 * xg.real).sum(axis=1)
            ai = (1.0 - mu) * np.abs(b0 * xg.imag).sum(axis=1) + mu * np.abs(b1 * xg.imag).sum(axis=1)
            A[r] = ar + 1j * ai
        else:
            A[r] = (1.0 - mu) * np.abs(b0 * xg).sum(axis=1) + mu * np.abs(b1 * xg).sum(axis=1)
    return (Y[0], A[0]) if one else (Y, A)


def _fma(a, b, c):
    """fmaf on f32 arrays: the product of two f32 is exact in f64; the sum is rounded to f64 and then to f32 (a double rounding
    that differs from fmaf in rare ties: good for a yardstick, not for a bit-exact model)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _yard_real(b0, b1, mu, xg):
    s0, s1 = np.zeros(xg.shape[0], f32), np.zeros(xg.shape[0], f32)
    for j in range(xg.shape[1]):
        s0 = _fma(b0[:, j], xg[:, j], s0)
        s1 = _fma(b1[:, j], xg[:, j], s1)
    mu = mu.astype(f32)                                   # 24 bits: exact
    return _fma(mu, s1, (f32(1.0) - mu) * s0)


def yardstick(bank, delta, x):
    rows, one = _rows(x)
    cplx = np.iscomplexobj(rows)
    bank = np.asarray(bank, f32)
    P = bank.shape[1]
    n_out = count(0, delta, rows.shape[1])
    nk, b, mu = times(0, delta, n_out)
    b0, b1 = bank[b], bank[b + 1]
    Y = np.empty((rows.shape[0], n_out), np.complex64 if cplx else f32)
    for r in range(rows.shape[0]):
        if cplx:
            xg = _gather(rows[r].astype(np.complex64), nk, P)
            Y[r] = _yard_real(b0, b1, mu, np.ascontiguousarray(xg.real)) + 1j * _yard_real(b0, b1, mu, np.ascontiguousarray(xg.imag))
        else:
            Y[r] = _yard_real(b0, b1, mu, _gather(rows[r].astype(f32), nk, P))
    return Y[0] if one else Y


def bound(A, P):
    return (P + 3) * U * A


def worst_ratio(got, ref, A, P):
    """max over the elements and components of |got - truth| / ((P + 3) 2^-24 A_k); an element whose bound is 0 has to be exact"""
    d = np.asarray(got).astype(ref.dtype) - ref
    parts = [(np.abs(d.real), bound(A.real, P)), (np.abs(d.imag), bound(A.imag, P))] if np.iscomplexobj(ref) else [(np.abs(d), bound(A, P))]
    worst = 0.0
    for e, bnd in parts:
        zero = bnd == 0
        if np.any(e[zero] != 0):
            return float("inf")
        if np.any(~zero):
            worst = max(worst, float((e[~zero] / bnd[~zero]).max()))
    return worst


def fskmod(sym, sps, bw_in):
    """2-FSK, phase-continuous, at `sps` samples per symbol (a real number): symbol i lasts from sample time i sps to (i + 1) sps
    and its tone sits at (2 sym - 1) bw_in cycles per sample; sample t takes the phase integrated up to t.  CF32 [floor(len sps)]"""
    sym = np.asarray(sym, np.int64)
    f = (2.0 * sym - 1.0) * float(bw_in)
    n = int(np.floor(sym.size * sps + 1e-9))
    t = np.arange(n, dtype=np.float64)
    i = np.minimum((t / sps).astype(np.int64), sym.size - 1)
    start = np.concatenate([[0.0], np.cumsum(f * sps)[:-1]])          # cycles at the start of each symbol
    return np.exp(2j * np.pi * (start[i] + f[i] * (t - i * sps))).astype(np.complex64)
