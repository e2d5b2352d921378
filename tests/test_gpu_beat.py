"""Beat-Transformer engine on the MI355X: reference parity (goldens), the numpy restatement at shapes the goldens lack, bitwise layout invariance and
reproducibility, and the Python surface (activations / forward / detect / input checks)."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beat_np  # noqa: E402

from etude_amd import _lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu
WEIGHT_SEED = 7


def _close(got, ref, what):
    bar = 1e-4 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    assert err <= bar, f"{what}: max |d| {err:.3e} > {bar:.3e}"


@pytest.fixture(scope="module")
def sd():
    return synth.beat_state_dict(WEIGHT_SEED)


@pytest.fixture(scope="module")
def det(sd):
    from etude_amd import BeatDetector
    return BeatDetector(state_dict=sd)


@pytest.fixture(scope="module")
def det_small(sd):
    from etude_amd import BeatDetector
    return BeatDetector(state_dict=sd, max_rows=2048)


def _fwd(d, feat):
    lg, tp = d.forward(torch.from_numpy(np.ascontiguousarray(feat))[None].cuda())
    torch.cuda.synchronize()
    return lg[0].cpu().numpy(), tp[0].cpu().numpy()


@pytest.mark.parametrize("T", [1, 5, 37, 300, 1100])
def test_reference_parity(golden_dir, det, T):
    g = np.load(golden_dir / f"beat_T{T}.npz")
    feat = synth.beat_features(int(g["seed"]), T)
    rows = 5 * T
    front = torch.zeros(rows, 256, device="cuda") if T == 37 else None
    l0 = torch.zeros(rows, 256, device="cuda") if T == 37 else None
    det.debug_taps(front, l0)
    try:
        lg, tp = _fwd(det, feat)
    finally:
        det.debug_taps(None, None)
    _close(lg, g["logits"], f"logits T={T}")
    _close(tp, g["tempo"], f"tempo T={T}")
    if T == 37:
        _close(front.view(5, T, 256).cpu().numpy(), g["front"], "front-end tap")
        _close(l0.view(5, T, 256).cpu().numpy(), g["layer0"], "layer-0 tap")


def test_reference_parity_batch(golden_dir, det):
    g = np.load(golden_dir / "beat_B2.npz")
    T = int(g["T"])
    x = torch.from_numpy(np.stack([synth.beat_features(int(s), T) for s in g["seeds"]])).cuda()
    lg, tp = det.forward(x)
    assert lg.shape == (2, T, 2) and tp.shape == (2, 300)
    _close(lg.cpu().numpy(), g["logits"], "B=2 logits")
    _close(tp.cpu().numpy(), g["tempo"], "B=2 tempo")


@pytest.mark.parametrize("T", [2, 3, 4, 1023, 1024, 1025, 2049])
def test_restatement_at_edge_shapes(sd, det, T):
    feat = synth.beat_features(1000 + T, T)
    lg, tp = _fwd(det, feat)
    r = beat_np.forward(sd, feat)
    _close(lg, r["logits"], f"logits T={T}")
    _close(tp, r["tempo"], f"tempo T={T}")


def test_restatement_full_song(sd, det):
    T = 7752                                  # 3 min at 44100 / 1024 fps
    feat = synth.beat_features(4242, T)
    lg, tp = _fwd(det, feat)
    r = beat_np.forward(sd, feat)
    _close(lg, r["logits"], "logits 3-min song")
    _close(tp, r["tempo"], "tempo 3-min song")


def _ragged(det, songs):
    feat = torch.cat([torch.from_numpy(s).reshape(-1) for s in songs]).cuda()
    Ts = [s.shape[1] for s in songs]
    lg, tp = det._run(feat, Ts)
    torch.cuda.synchronize()
    lg, tp = lg.cpu().numpy(), tp.cpu().numpy()
    out, o = [], 0
    for i, T in enumerate(Ts):
        out.append((lg[o:o + T].copy(), tp[i].copy()))
        o += T
    return out


def test_layout_invariance_bitwise(det, det_small):
    Ts = [37, 1, 300, 1025, 5, 64, 2049]
    songs = [synth.beat_features(500 + i, T) for i, T in enumerate(Ts)]
    solo = [_fwd(det, s) for s in songs]
    batch = _ragged(det, songs)
    order = [6, 2, 0, 5, 3, 1, 4]
    rev = _ragged(det, [songs[i] for i in order])
    chunked = _ragged(det_small, songs)          # 2048 rows per chunk: several chunks, and the 2049-frame song alone exceeds it
    for i in range(len(Ts)):
        for name, (lg, tp) in (("batch", batch[i]), ("reordered", rev[order.index(i)]), ("chunked", chunked[i])):
            assert np.array_equal(lg, solo[i][0]), (name, Ts[i])
            assert np.array_equal(tp, solo[i][1]), (name, Ts[i])


def test_reproducible_and_no_state_leak(sd, det):
    from etude_amd import BeatDetector
    short = synth.beat_features(77, 41)
    long_ = synth.beat_features(78, 3000)
    a = _fwd(det, short)
    b = _fwd(det, short)
    _fwd(det, long_)
    c = _fwd(det, short)
    other = BeatDetector(state_dict=sd)
    d = _fwd(other, short)
    for x in (b, c, d):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])


def test_activations_are_sigmoid_of_forward(det):
    feat = synth.beat_features(9, 400)
    beat, down = det.activations(feat)
    assert beat.dtype == np.float32 and down.dtype == np.float32 and beat.shape == (400,)
    lg, _ = det.forward(torch.from_numpy(feat)[None].cuda())
    s = torch.sigmoid(lg[0]).cpu().numpy()
    assert np.array_equal(beat, s[:, 0]) and np.array_equal(down, s[:, 1])
    many = det.activations_many([feat, synth.beat_features(10, 50)])
    assert np.array_equal(many[0][0], beat) and np.array_equal(many[0][1], down) and many[1][0].shape == (50,)


def test_bad_features_refused_before_launch(det):
    _lib.prof_enable(True)
    try:
        _lib.prof_reset()
        for bad in (np.full((5, 20, 128), -81.0, np.float32), np.full((5, 20, 128), np.nan, np.float32)):
            with pytest.raises(ValueError):
                det.activations(bad)
            with pytest.raises(ValueError):
                det.forward(torch.from_numpy(bad)[None].cuda())
        with pytest.raises(ValueError):
            det.activations_many([synth.beat_features(1, 10), np.full((5, 10, 128), np.inf, np.float32)])
        assert not [k for k in _lib.prof_report() if "beat" in k or "gemm3" in k]
    finally:
        _lib.prof_enable(False)


class _StubBeat:
    def __init__(self):
        self.seen = None

    def __call__(self, act):
        self.seen = act.copy()
        return np.array([0.5, 1.0, 1.5])


class _StubDown:
    def __init__(self):
        self.seen = None

    def __call__(self, act):
        self.seen = act.copy()
        return np.array([[0.5, 1.0], [1.0, 2.0], [1.5, 1.0]])


def test_detect_with_stub_trackers(tmp_path, det, monkeypatch):
    feat = synth.beat_features(11, 120)
    p = tmp_path / "song.npy"
    np.save(p, feat)
    sb, sdn = _StubBeat(), _StubDown()
    monkeypatch.setattr(det, "_trackers", lambda: (sb, sdn))
    out = tmp_path / "sub" / "tempo.json"
    res = det.detect(p, out, cleanup_input=False)
    assert p.exists()
    assert res == {"beat_pred": [0.5, 1.0, 1.5], "downbeat_pred": [0.5, 1.5]}
    assert json.loads(out.read_text()) == res
    beat, down = det.activations(feat)
    assert np.array_equal(sb.seen, beat)
    assert np.array_equal(sdn.seen, np.stack([np.maximum(beat - down, 0), down], axis=-1))
    det.detect(p)
    assert not p.exists()


def test_detect_without_madmom_names_it(tmp_path, det):
    try:
        import madmom  # noqa: F401
        pytest.skip("madmom is installed here")
    except ImportError:
        pass
    p = tmp_path / "x.npy"
    np.save(p, synth.beat_features(1, 10))
    with pytest.raises(ImportError, match="madmom"):
        det.detect(p)
    assert p.exists()
