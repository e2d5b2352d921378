"""DESIGN.md 4g restated in numpy: mono audio at 22 050 Hz -> (tuning in cents, sim[100]).  fp64 by default; every stage takes ``dtype=np.float32`` and then runs in
float32 with the same fixed order of the sum over time (the E32 reference of tests/test_gpu_tuning.py).  The spline is a tridiagonal solve of its own (no scipy).
Also the fixtures the host and the device tests share."""
import numpy as np

FS = 22050
N_FFT = 16384
HOP = 8192
BINS = N_FFT // 2 + 1
GROUP = 8
LOGF = 8400
THETA = 100
AVG = 50
COMB = 84
MIN_N = 2 * N_FFT
H = FS / N_FFT                                        # knot spacing in Hz (exact in binary)
F24 = 440.0 * 2.0 ** ((24 - 69) / 12)


def num_frames(N):
    if N < MIN_N:
        raise ValueError(f"estimate_tuning: N = {N} is shorter than two windows ({MIN_N})")
    return 1 + N // HOP


def window():
    """the periodic Hann of 16 384 points, formed in fp64, the float32 table the device is handed"""
    n = np.arange(N_FFT, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)).astype(np.float32)


def frames(x, which=None, dtype=np.float64):
    """step 1: frame f is x[8192 (f - 1) + n] times the window, zero outside the signal -> [len(which)][16384].  The product is formed in `dtype` (float32 samples
    times the float32 table)."""
    x = np.asarray(x, np.float32)
    F = num_frames(len(x))
    which = range(F) if which is None else which
    xp = np.concatenate([np.zeros(HOP, np.float32), x, np.zeros(N_FFT, np.float32)])
    w = window().astype(dtype)
    return np.stack([xp[HOP * f: HOP * f + N_FFT].astype(dtype) * w for f in which])


def _fft32(fr):
    """a radix-2 decimation-in-time FFT in complex64 (float32 arithmetic, twiddles rounded from fp64) over the last axis: the float32 counterpart of numpy's fp64 rfft"""
    n = fr.shape[-1]
    lg = n.bit_length() - 1
    rev = np.zeros(n, np.int64)
    for b in range(lg):
        rev |= ((np.arange(n) >> b) & 1) << (lg - 1 - b)
    z = fr.astype(np.complex64)[..., rev]
    for s in range(lg):
        half = 1 << s
        tw = np.exp(-2j * np.pi * np.arange(half) / (2 * half)).astype(np.complex64)
        z = z.reshape(fr.shape[:-1] + (n // (2 * half), 2, half))
        a, b = z[..., 0, :], z[..., 1, :] * tw
        z = np.stack([a + b, a - b], axis=-2).reshape(fr.shape[:-1] + (n,))
    return z[..., : n // 2 + 1]


def power(fr, dtype=np.float64):
    """step 2a: P[f][k] = re^2 + im^2 of the real DFT, k = 0 .. 8192"""
    if dtype == np.float64:
        X = np.fft.rfft(np.asarray(fr, np.float64), axis=-1)
        return X.real ** 2 + X.imag ** 2
    X = _fft32(np.asarray(fr, np.float32))
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    return re * re + im * im


def compress(P, dtype=np.float64):
    """step 2b: C = log(1 + 100 P)"""
    P = np.asarray(P, dtype)
    return np.log(dtype(1) + dtype(100) * P).astype(dtype)


def time_sum(C, dtype=np.float64):
    """step 3: Y[k] = sum over groups ascending of (sum over the group's frames ascending of C[f][k]); group g = frames 8 g .. min(F, 8 g + 8) - 1"""
    C = np.asarray(C, dtype)
    Y = None
    for g0 in range(0, C.shape[0], GROUP):
        part = C[g0].copy()
        for f in range(g0 + 1, min(C.shape[0], g0 + GROUP)):
            part = part + C[f]
        Y = part if Y is None else Y + part
    return Y.astype(dtype)


def spectrum_sum(x, dtype=np.float64):
    """steps 1-3 of a song -> Y [8193]"""
    return time_sum(compress(power(frames(x, dtype=dtype), dtype), dtype), dtype)


def pivots():
    """the elimination of the spline's tridiagonal system on uniform knots depends on the knots alone: (reciprocal pivots rp, scaled upper diagonal cp), fp64 [8193]"""
    n = BINS
    rp, cp = np.zeros(n), np.zeros(n)
    rp[0], cp[0] = 1.0, 2.0
    for i in range(1, n - 1):
        rp[i] = 1.0 / (4.0 - cp[i - 1])
        cp[i] = rp[i]
    rp[n - 1] = 1.0 / (1.0 - 2.0 * cp[n - 2])
    return rp, cp


def log_axis():
    """fl[i] = f24 2^(i / 1200), i < 8400; the knot interval of each and the offset inside it"""
    fl = F24 * 2.0 ** (np.arange(LOGF) / 1200.0)
    iv = np.minimum(np.floor(fl / H).astype(np.int64), BINS - 2)
    return fl, iv, fl - iv * H


def knot_derivatives(Y, dtype=np.float64):
    """the not-a-knot cubic spline through (k h, Y[k]) in its first-derivative form: rows d_0 + 2 d_1 = (5 s_0 + s_1) / 2, d_{i-1} + 4 d_i + d_{i+1} = 3 (s_{i-1} + s_i),
    2 d_{n-2} + d_{n-1} = (s_{n-3} + 5 s_{n-2}) / 2 with s_j = (Y[j+1] - Y[j]) / h; forward elimination, then back substitution"""
    Y = np.asarray(Y, dtype)
    n = len(Y)
    h = dtype(H)
    s = (Y[1:] - Y[:-1]) / h
    b = np.empty(n, dtype)
    b[0] = (dtype(5) * s[0] + s[1]) / dtype(2)
    b[1:-1] = dtype(3) * (s[:-1] + s[1:])
    b[-1] = (s[-2] + dtype(5) * s[-1]) / dtype(2)
    rp, cp = (t.astype(dtype) for t in pivots())
    d = np.empty(n, dtype)
    prev = b[0] * rp[0]
    d[0] = prev
    for i in range(1, n - 1):
        prev = (b[i] - prev) * rp[i]
        d[i] = prev
    prev = (b[n - 1] - dtype(2) * prev) * rp[n - 1]
    d[n - 1] = prev
    for i in range(n - 2, -1, -1):
        prev = d[i] - cp[i] * prev
        d[i] = prev
    return d


def log_frequency(Y, dtype=np.float64):
    """step 4: the spline evaluated at fl -> Yi [8400]"""
    Y = np.asarray(Y, dtype)
    d = knot_derivatives(Y, dtype)
    _, iv, tt = log_axis()
    t, h = tt.astype(dtype), dtype(H)
    y0, s, d0, d1 = Y[iv], (Y[iv + 1] - Y[iv]) / h, d[iv], d[iv + 1]
    c2 = (dtype(3) * s - dtype(2) * d0 - d1) / h
    c3 = (d0 + d1 - dtype(2) * s) / (h * h)
    return (y0 + t * (d0 + t * (c2 + t * c3))).astype(dtype)


def rectify(Yi, dtype=np.float64):
    """step 5: R = max(0, Yi - S), S the 101-point local average with zeros outside, summed with j ascending"""
    Yi = np.asarray(Yi, dtype)
    pad = np.concatenate([np.zeros(AVG, dtype), Yi, np.zeros(AVG, dtype)])
    acc = np.zeros(LOGF, dtype)
    for j in range(2 * AVG + 1):
        acc = acc + pad[j: j + LOGF]
    S = acc * dtype(1.0 / (2 * AVG + 1))
    return np.maximum(dtype(0), Yi - S).astype(dtype)


def comb(R, dtype=np.float64):
    """step 6: sim[theta + 50] = sum over m = 0 .. 83 ascending of R[100 m + theta], indices inside [0, 8400) only"""
    R = np.asarray(R, dtype)
    sim = np.zeros(THETA, dtype)
    for m in range(COMB):
        idx = 100 * m + np.arange(-THETA // 2, THETA // 2)
        ok = (idx >= 0) & (idx < LOGF)
        sim[ok] = sim[ok] + R[idx[ok]]
    return sim


def tuning_of(sim):
    return int(np.argmax(sim)) - THETA // 2


def estimate(x, dtype=np.float64):
    """-> (tuning, dict of every stage)"""
    Y = spectrum_sum(x, dtype)
    Yi = log_frequency(Y, dtype)
    R = rectify(Yi, dtype)
    sim = comb(R, dtype)
    return tuning_of(sim), dict(Y=Y, Yi=Yi, R=R, sim=sim)


def margin(sim):
    """(sim[best] - sim[second]) / sim[best]"""
    s = np.sort(np.asarray(sim, np.float64))
    return float((s[-1] - s[-2]) / s[-1])


# ---- fixtures shared by the CPU and the GPU tests
def planted_song(seed, N, cents, amp=0.1):
    """seeded decaying notes -- harmonics 1-3 at amplitudes 1, 0.5, 0.25, decay exp(-3 t), four notes per second at pitches 40 .. 89 -- every pitch `cents` off equal
    temperament, over noise of 1e-3: mono float32 [N]"""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / FS
    x = 1e-3 * rng.standard_normal(N)
    for i in range(int(np.ceil(4 * N / FS))):
        p, t0 = int(rng.integers(40, 90)), i / 4.0
        f = 440.0 * 2.0 ** ((p - 69 + cents / 100.0) / 12.0)
        n0 = int(np.ceil(t0 * FS))
        tt = t[n0:] - t0
        env = np.exp(-3.0 * tt)
        for k, g in ((1, 1.0), (2, 0.5), (3, 0.25)):
            x[n0:] += amp * g * env * np.sin(2 * np.pi * k * f * tt)
    return x.astype(np.float32)


def sinusoid(N, cents, pitch=69, amp=0.3):
    t = np.arange(N) / FS
    return (amp * np.sin(2 * np.pi * 440.0 * 2.0 ** ((pitch - 69 + cents / 100.0) / 12.0) * t)).astype(np.float32)


# (seed, N, planted cents) of the host tests of the estimate
PLANTED = ((11, 8 * FS, 0), (12, 8 * FS, -37), (13, 8 * FS, 23), (14, 8 * FS, 49), (15, 8 * FS, -50), (16, 32790, 12), (17, 30 * FS, -8))
# (seed, N, planted cents) of every seeded input whose stages and integer the device tests check: a partial group, 40 959, exactly one group, the first group edge,
# 17 frames, an 8-second song, a detuned one
DEVICE_INPUTS = ((21, 32768, 0), (22, 40959, 5), (23, 57344, -20), (24, 65536, 31), (25, 131072, -44), (11, 8 * FS, 0), (12, 8 * FS, -37))
# the short songs of the bank-split test: 70 sinusoids, each its own number of cents off (more than the 64 filterbanks of one alignfeat handle).  Pitch 100
# (2 637 Hz): there a bin of 1.35 Hz is 0.9 cents, so every one of the 70 detunings gets an estimate of its own (at pitch 69 a bin is 5.3 cents and they fall into 37)
SPLIT_CENTS = tuple(range(-35, 35))
SPLIT_N = 32768
SPLIT_PITCH = 100


def split_songs():
    return [sinusoid(SPLIT_N, d, pitch=SPLIT_PITCH) for d in SPLIT_CENTS]

# the chain fixture: 4f's planted warp with both renderings this many cents flat
CHAIN_CENTS = -30
# the host restatement of that chain (estimate -> features at the estimated offset -> dtw_np) puts the path within this many origin frames of the planted warp
# (measured on the host, tests/test_tuning_cpu.py; asserted at twice that there and in the device chain test, as 4f does)
CHAIN_MEASURED = 2.410
CHAIN_BOUND = 2 * CHAIN_MEASURED


def chain_audio(cents=CHAIN_CENTS):
    """4f's planted-warp fixture (alignfeat_np.planted_warp_audio: same seed, notes and warp) with every pitch of both renderings `cents` off equal temperament
    -> (cover, origin, warp, transpose).  The fixture is rendered by its own code: only the pitches its renderer is handed are shifted."""
    import alignfeat_np as an
    render = an.render_roll
    an.render_roll = lambda notes, N: render([(p + cents / 100.0, t0, a) for p, t0, a in notes], N)
    try:
        return an.planted_warp_audio()
    finally:
        an.render_roll = render
