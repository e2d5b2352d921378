"""The piano voice of DESIGN.md 4l restated in numpy, from its formulas alone: the yardstick of csrc/render.hip.

``render_np(notes, sr, cents, voice, num_samples=None, dtype=np.float64)`` -> (samples, envelope sum).  The envelope sum is the same sum with every sine replaced by
1: it bounds |x| and scales the device's tolerance.

dtype=np.float32 is what a careful fp32 implementation can reach: the time base stays fp64 -- the seconds since the onset and since the offset, and the phase in
revolutions f_k (n / sr - onset), reduced to [-0.5, 0.5) -- and everything behind it is float32: the rounding of the reduced phase and of the two times, the sine
(of float32(2 pi) times the phase), the envelope, the products and the sums.
"""
import math

import numpy as np

from etude_amd.render import PianoVoice

NOTE_FIELDS = ("onset", "offset", "pitch", "velocity")


def note_tuples(notes):
    """any of the accepted in-memory forms -> [(onset, offset, pitch, velocity)], stably sorted by onset"""
    if isinstance(notes, np.ndarray):
        rows = [tuple(float(n[f]) if f in ("onset", "offset") else int(n[f]) for f in NOTE_FIELDS) for n in notes]
    else:
        rows = [tuple(n[f] for f in NOTE_FIELDS) if isinstance(n, dict) else tuple(n) for n in notes]
    return sorted(rows, key=lambda r: r[0])      # (sorted() is stable)


def partials(pitch, velocity, cents, sr, voice=PianoVoice()):
    """-> (f_k [K'], A_k [K'], T_k [K']) of the partials that exist at this rate, fp64"""
    f0 = 440.0 * 2.0 ** ((pitch - 69) / 12.0 + cents / 1200.0)
    B = voice.inharmonicity * 2.0 ** ((pitch - 60) / voice.inharmonicity_step)
    T = voice.decay_base * 2.0 ** (-(pitch - 21) / voice.decay_halving)
    f, A, Tk = [], [], []
    for k in range(1, voice.partials + 1):
        fk = k * f0 * math.sqrt(1.0 + B * k * k)
        if fk >= voice.nyquist_fraction * sr:
            continue
        f.append(fk)
        A.append((velocity / 127.0) ** voice.velocity_power * k ** (-voice.partial_rolloff))
        Tk.append(T / (1.0 + voice.decay_partial * (k - 1)))
    return np.array(f), np.array(A), np.array(Tk)


def length_of(notes, sr, voice=PianoVoice()):
    """N = ceil((max offset + R) sr) + 1; 0 without notes"""
    rows = note_tuples(notes)
    if not rows:
        return 0
    return int(math.ceil((max(r[1] for r in rows) + voice.support) * sr)) + 1


def render_np(notes, sr=22050, cents=0.0, voice=PianoVoice(), num_samples=None, dtype=np.float64):
    rows = note_tuples(notes)
    N = length_of(rows, sr, voice) if num_samples is None else int(num_samples)
    dt = np.dtype(dtype).type
    x, env = np.zeros(N, dt), np.zeros(N, dt)
    R = voice.support
    for onset, offset, pitch, velocity in rows:
        lo = max(0, int(math.floor(onset * sr)) - 1)
        hi = min(N, int(math.ceil((offset + R) * sr)) + 2)      # a window that holds the note's samples; the predicates below decide
        if hi <= lo:
            continue
        n = np.arange(lo, hi, dtype=np.float64)
        t = n / sr
        tau, u = t - onset, t - offset                           # fp64: the time base
        on = (tau >= 0) & (u < R)
        tau_t, u_t = tau.astype(dt), u.astype(dt)
        g = np.minimum(tau_t / dt(voice.attack), dt(1))
        if voice.release:
            with np.errstate(over="ignore"):
                rel = np.exp(-(u_t / dt(voice.release_tau))) * (dt(1) - u_t / dt(voice.release_len))
            g = g * np.where(u_t > 0, rel, dt(1))
        f, A, Tk = partials(pitch, velocity, cents, sr, voice)
        s, e = np.zeros(len(n), dt), np.zeros(len(n), dt)
        for k in range(len(f)):
            ph = f[k] * tau                                      # revolutions, fp64
            r = (ph - np.floor(ph + 0.5)).astype(dt)             # [-0.5, 0.5), then the working precision
            a = np.full(len(n), dt(A[k]))
            if voice.decay:
                with np.errstate(over="ignore"):
                    a = a * np.exp(-(tau_t / dt(Tk[k])))
            s = s + a * np.sin(dt(2.0 * math.pi) * r)
            e = e + a
        idx = np.nonzero(on)[0] + lo
        x[idx] = x[idx] + (g * s)[on]
        env[idx] = env[idx] + (g * e)[on]
    return dt(voice.gain) * x, dt(voice.gain) * env


def first_end(onset, offset, sr, voice=PianoVoice()):
    """the samples a note sounds on, by the predicates above: (first n with n / sr >= onset, first n with n / sr - offset >= R)"""
    R = voice.support
    n = np.arange(max(0, int(onset * sr) - 2), int((offset + R) * sr) + 4, dtype=np.float64)
    t = n / sr
    return int(n[np.argmax(t - onset >= 0)]), int(n[np.argmax(t - offset >= R)])
