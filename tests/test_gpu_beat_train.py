"""The Beat-Transformer training engine (etude_amd.BeatTrainer, csrc/beat_train.hip) against fp64 autograd of the restatement (tests/beat_train_np.py).

The yardstick is DESIGN.md 4j's rule, not a constant: every device figure is ``err = max|g - g64| / max|g64|`` per tensor and is held to 4 x the same figure of fp32
torch on the CPU for the same loss on the same batch, never asked below 4 * 2^-24.  Where fp64 autograd gives an exact zero (head 7's key rows, the tempo head without
a tempo target, masked taps of Er at T = 1) the device must give an exact zero too.  Measured figures: profiles/beat_train_device.json, DESIGN.md 4s
(ETD_BEAT_TRAIN_REPORT=dir keeps them as JSON).

The T = 1030 case takes features that are periodic in time (3 frames repeated).  The front end's three max-pools route a gradient to the larger of values that
fp32 cannot always tell apart: on 1030 frames of aperiodic features the fp64 restatement has 26 conv3 cells whose top two values lie within 1e-6 (the closest within
3e-9) while fp32 torch's own conv3 output is off by up to 5e-6, and flipping those choices in the fp64 restatement moves the conv gradients by 2e-5 -- any fp32
implementation, fp32 torch included, then meets or misses fp64 by luck, whatever its kernels do.  With 3 distinct frames (plus the edges) there are few enough cells to
find a seed at which every choice is decidable; the test asserts it on the restatement: every top-2 gap and every distance of a maximum from the ReLU's kink is above
twice fp32 torch's largest error of that pool's input.  Because period 3 makes the row 1024 frames back look like the row 1 frame back, the APERIODIC 1030-frame
input is kept as a case of its own (``l9_T1030_aperiodic``): every tensor is held to the bound except the five whose gradient passes through the pool choices
(conv1 / conv2 / conv3 weights, conv1 / conv2 biases), which the periodic case holds; its figures for those five are printed, not asserted.
tools/beat_pool_flip.py reproduces the experiment quoted above.

The stage edges of single kernels, on inputs of their own between guard floats, are tests/test_gpu_beat_train_stages.py.
"""
import json
import os

import numpy as np
import pytest
import torch

import beat_np
import beat_train_np as bt
from etude_amd import synth
from etude_amd.config import BeatDetectorConfig, BeatDetectorModelConfig

pytestmark = pytest.mark.gpu

FLOOR = 4.0 * 2.0 ** -24
OPT = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.5)
LOSS = dict(pos_weight=(3.0, 7.0, 2.0), tempo_weight=0.5)
# name: architecture overrides, weight seed, batch seed, song lengths, songs without a tempo target, songs with every beat cell unscored, period of the features (0: none)
CASES = {
    "default_ragged": (dict(), 7, 31, (1, 2, 5, 37, 129, 300), (2,), (3,), 0),
    "archA": (dict(instr=3, nlayers=5, d_hid=512, ntoken=3), 11, 32, (3, 70), (), (), 0),
    "instr8_l11": (dict(instr=8, nlayers=11, d_hid=256), 12, 33, (40,), (), (), 0),
    "l9_T1030": (dict(nlayers=9, d_hid=256), 13, 142, (1030,), (), (), 3),       # the smallest T at which head 4's tap at -4 * 256 is in range
    "l9_T1030_aperiodic": (dict(nlayers=9, d_hid=256), 13, 34, (1030,), (), (), 0),
    "one_row": (dict(instr=1, nlayers=9, d_hid=256), 14, 35, (1,), (), (), 0),
}


# the tensors whose gradient passes through the front end's max-pool choices (conv3.bias does not: the routed column does not change a column sum)
POOL_DOWNSTREAM = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight")


def model_config(over):
    d = synth.beat_dims(**over)
    return BeatDetectorModelConfig(attn_len=5, instr=d["instr"], ntoken=d["ntoken"], dmodel=256, nhead=8, d_hid=d["d_hid"], nlayers=d["nlayers"], norm_first=True), d


def loss_kw(ntoken):
    return dict(pos_weight=LOSS["pos_weight"][:ntoken], tempo_weight=LOSS["tempo_weight"])


def trainer(cfg, state, max_rows, **kw):
    from etude_amd import BeatTrainer
    return BeatTrainer(cfg, state, max_rows=max_rows, max_seqs=8, **OPT, **loss_kw(cfg.ntoken), **kw)


def report(name, rows):
    for r in rows:
        print(name, r)
    out = os.environ.get("ETD_BEAT_TRAIN_REPORT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(rows, f, indent=1)


def args_of(batch):
    return batch["feats"], batch["beat"], batch["tempo"]


@pytest.mark.parametrize("name", list(CASES))
def test_whole_gradient_against_fp64_autograd(name):
    over, wseed, bseed, Ts, no_tempo, unscored, period = CASES[name]
    cfg, dims = model_config(over)
    state = synth.beat_state_dict(wseed, dims)
    batch = bt.make_batch(bseed, Ts, instr=cfg.instr, ntoken=cfg.ntoken, no_tempo=no_tempo, unscored=unscored, period=period)
    if period:      # every max-pool choice is decidable in fp32 (module docstring)
        for f in batch["feats"]:
            for m in bt.pool_margins(state, f):
                assert min(m["gap"], m["kink"]) > 2.0 * m["err32"], m
    kw = loss_kw(cfg.ntoken)
    l64, g64 = bt.loss_and_grads(state, cfg.nlayers, batch, torch.float64, **kw)
    l32, g32 = bt.loss_and_grads(state, cfg.nlayers, batch, torch.float32, **kw)
    tr = trainer(cfg, state, max_rows=cfg.instr * sum(Ts))
    try:
        loss, n_scored, skipped = tr.loss_and_backward(*args_of(batch))
        g = tr.grads()
    finally:
        tr.close()
    assert not skipped and n_scored == sum(int((y >= 0).sum()) for y in batch["beat"])
    rows, bad = [], []
    e_loss, e_loss32 = abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    rows.append(dict(tensor="loss", err=e_loss, err32=e_loss32))
    if not e_loss <= max(4.0 * e_loss32, FLOOR):
        bad.append(("loss", e_loss, e_loss32))
    for k, r in g64.items():
        zero = r == 0
        if zero.any() and np.any(g[k][zero] != 0):
            bad.append((k, "nonzero where fp64 is exactly zero", float(np.abs(g[k][zero]).max())))
        e, e32 = bt.rel_err(g[k], r), bt.rel_err(g32[k], r)
        rows.append(dict(tensor=k, err=e, err32=e32, ratio=e / max(e32, 2.0 ** -24)))
        if name == "l9_T1030_aperiodic" and k in POOL_DOWNSTREAM:
            continue                                    # held by l9_T1030 (module docstring); printed with the other figures
        if not e <= max(4.0 * e32, FLOOR):
            bad.append((k, e, e32))
    rows.sort(key=lambda r: -r.get("ratio", 0.0))
    report("whole_" + name, rows)
    assert not bad, bad[:12]


@pytest.fixture(scope="module")
def small():
    cfg, dims = model_config(dict(instr=3, nlayers=5, d_hid=512, ntoken=3))
    state = synth.beat_state_dict(11, dims)
    batch = bt.make_batch(41, (17, 33), instr=3, ntoken=3, no_tempo=(1,))
    return dict(cfg=cfg, state=state, batch=batch)


def test_same_call_same_bits(small):
    out = []
    for _ in range(2):
        tr = trainer(small["cfg"], small["state"], 256)
        try:
            loss = tr.loss_and_backward(*args_of(small["batch"]))[0]
            out.append((loss, tr.grads()))
        finally:
            tr.close()
    assert out[0][0] == out[1][0]
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k].view(np.uint32), out[1][1][k].view(np.uint32)), k


def test_accumulation_is_one_add_per_call(small):
    """two calls with loss_scale 0.5: the accumulated gradient is fl(g_1 + g_2) of the two calls' own gradients (each formed from zero), element by element"""
    b1 = small["batch"]
    b2 = bt.make_batch(42, (9, 40), instr=3, ntoken=3)
    tr = trainer(small["cfg"], small["state"], 256)
    try:
        singles = []
        for b in (b1, b2):
            tr.zero_grad()
            tr.loss_and_backward(*args_of(b), loss_scale=0.5)
            singles.append(tr.grads())
        tr.zero_grad()
        for b in (b1, b2):
            tr.loss_and_backward(*args_of(b), loss_scale=0.5)
        both = tr.grads()
    finally:
        tr.close()
    for k in both:
        want = singles[0][k] + singles[1][k]
        assert np.array_equal(both[k].view(np.uint32), want.view(np.uint32)), k


def test_skipped_batch_launches_nothing_and_keeps_every_bit(small):
    b = small["batch"]
    tr = trainer(small["cfg"], small["state"], 256)
    try:
        tr.loss_and_backward(*args_of(b))
        before = tr.grads()
        nothing = [np.full_like(y, -1.0) for y in b["beat"]]
        loss, n_scored, skipped = tr.loss_and_backward(b["feats"], nothing, None)
        after = tr.grads()
    finally:
        tr.close()
    assert np.isnan(loss) and n_scored == 0 and skipped
    for k in before:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k


def test_refusals_on_the_device_path(small):
    from etude_amd import _lib
    tr = trainer(small["cfg"], small["state"], 60)
    try:
        b = small["batch"]                              # 3 x (17 + 33) = 150 rows > 60
        with pytest.raises(_lib.EtudeHipError, match="max_rows"):
            tr.loss_and_backward(*args_of(b))
        assert all(not v.any() for v in tr.grads().values())
    finally:
        tr.close()


def test_ten_steps_follow_the_fp64_trajectory(small):
    """one ragged batch split in two (accumulation 2), ten optimizer steps: the losses stay within 4 x fp32 torch's own deviation from the fp64 trajectory"""
    cfg, state = small["cfg"], small["state"]
    batches = [small["batch"], bt.make_batch(43, (21,), instr=3, ntoken=3)]
    kw = loss_kw(cfg.ntoken)
    t64, _ = bt.trajectory(state, cfg.nlayers, batches, 10, torch.float64, **OPT, **kw)
    t32, _ = bt.trajectory(state, cfg.nlayers, batches, 10, torch.float32, **OPT, **kw)
    tr = trainer(cfg, state, 256)
    try:
        dev = [tr.train_step([args_of(b) for b in batches])[0] for _ in range(10)]
    finally:
        tr.close()
    t64, t32, dev = np.array(t64), np.array(t32), np.array(dev)
    e32 = float((np.abs(t32 - t64) / np.abs(t64)).max())
    e = float((np.abs(dev - t64) / np.abs(t64)).max())
    report("trajectory", [dict(err=e, err32=e32, first=float(t64[0, 0]), last=float(t64[-1, 0]))])
    assert t64[-1].sum() < t64[0].sum()                 # it learns
    assert e <= max(4.0 * e32, FLOOR), (e, e32)


def test_to_detector_is_the_saved_checkpoint(small, tmp_path):
    from etude_amd import BeatDetector
    cfg, state, b = small["cfg"], small["state"], small["batch"]
    tr = trainer(cfg, state, 256)
    try:
        tr.train_step([args_of(b)])
        path = tmp_path / "beat.pt"
        tr.save(path)
        trained = tr.state_dict()
        d1 = tr.to_detector()
        d2 = BeatDetector(BeatDetectorConfig(model=cfg), model_path=path, device="cuda")
        x = torch.from_numpy(np.stack([synth.beat_features(77, 50, instr=cfg.instr)]))
        l1, t1 = d1.forward(x)
        l2, t2 = d2.forward(x)
        assert torch.equal(l1, l2) and torch.equal(t1, t2)
        assert any(np.any(trained[k] != state[k]) for k in state)
        want = beat_np.forward(trained, x[0].numpy(), nlayers=cfg.nlayers)["logits"]
        got = l1[0].cpu().numpy()
        assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
        d1.close(); d2.close()
    finally:
        tr.close()


def test_key_bias_gradients_are_exactly_zero(small):
    """a key bias shifts every logit of a query alike: the engine leaves its gradient at exactly zero, the other two thirds of the same tensors are not"""
    tr = trainer(small["cfg"], small["state"], 256)
    try:
        tr.loss_and_backward(*args_of(small["batch"]))
        g = tr.grads()
    finally:
        tr.close()
    for l in range(small["cfg"].nlayers):
        p = f"Transformer_layers.time_attention_{l}.self_attn."
        assert not g[p + "key.bias"].any(), l
        assert g[p + "value.bias"].any() and (l >= 4 or g[p + "query.bias"].any()), l
        if 3 <= l <= 5:
            b = g[f"Transformer_layers.instr_attention_{l}.self_attn.in_proj_bias"]
            assert not b[256:512].any() and b[:256].any() and b[512:].any(), l


def test_a_song_alone_and_batched_has_the_same_rows():
    """The per-row results of a song -- its logits, the gradient of its front-end tokens (after every layer's backward) and the gradient of its conv1 rows (after the
    conv backward) -- are bit-identical alone and in the middle of a ragged batch.  The batch-level sums are made equal on purpose: 16 scored cells per class alone
    with loss_scale 0.5 against 32 in the batch with loss_scale 1, one tempo target alone against two in the batch."""
    cfg, dims = model_config(dict(instr=3, nlayers=5, d_hid=256))
    state = synth.beat_state_dict(21, dims)
    Ts = (21, 33, 9)
    batch = bt.make_batch(51, Ts, instr=3, ntoken=2, no_tempo=(2,))
    rng = np.random.default_rng(52)
    for s, n in ((0, 8), (1, 16), (2, 8)):              # exactly n scored cells per class
        y = batch["beat"][s]
        for c in range(2):
            col = np.full(Ts[s], -1.0, np.float32)
            at = rng.choice(Ts[s], n, replace=False)
            col[at] = rng.choice(np.array([0.0, 1.0, 0.5], np.float32), n)
            y[:, c] = col
    out = {}
    tr = trainer(cfg, state, 256)
    try:
        loss, n_scored, _ = tr.loss_and_backward([batch["feats"][1]], [batch["beat"][1]], [batch["tempo"][1]], loss_scale=0.5)
        assert n_scored == 32
        out["alone"] = [tr.debug_read_rows(w) for w in range(3)]
        tr.zero_grad()
        loss, n_scored, _ = tr.loss_and_backward(*args_of(batch), loss_scale=1.0)
        assert n_scored == 64
        out["batch"] = [tr.debug_read_rows(w) for w in range(3)]
    finally:
        tr.close()
    r0, f0 = 3 * Ts[0], Ts[0]
    for w, (lo, n) in enumerate(((r0, 3 * Ts[1]), (f0, Ts[1]), (r0, 3 * Ts[1]))):
        a, b = out["alone"][w], out["batch"][w][lo:lo + n]
        assert a.shape == b.shape and np.abs(a).max() > 0
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ("rows", w)


# ------------------------------------------------------------------ the parameter store: refusals of the read / write entries, checkpoint round trip
@pytest.fixture(scope="module")
def mini():
    """four layers, so that one instrument layer and its parameters exist; songs of 2 and 7 frames, the second with a tempo target"""
    cfg, dims = model_config(dict(instr=2, nlayers=4, d_hid=256))
    return dict(cfg=cfg, state=synth.beat_state_dict(15, dims), batch=bt.make_batch(43, (2, 7), instr=2, ntoken=cfg.ntoken, no_tempo=(0,)))


def test_read_and_write_refuse_unknown_names_wrong_sizes_and_unknown_buffers(mini):
    from etude_amd import _lib
    tr = trainer(mini["cfg"], mini["state"], 18)
    l, key = _lib.lib(), b"Transformer_layers.instr_attention_3.norm1.bias"
    n = mini["state"][key.decode()].size
    buf = np.zeros(n + 1, np.float32)
    try:
        with torch.cuda.device(tr.device):
            st = tr._stream(tr.device)
            for name in ("etd_btrain_read", "etd_btrain_write"):
                fn = getattr(l, name)
                for which in range(4):
                    with pytest.raises(_lib.EtudeHipError, match=r"etd_btrain: no parameter 'no\.such\.weight'"):
                        _lib.check(fn(tr.h, b"no.such.weight", which, buf.ctypes.data, n, st), name)
                    with pytest.raises(_lib.EtudeHipError, match=rf"etd_btrain: '{key.decode()}' has {n} elements, the buffer {n + 1}".replace(".", r"\.")):
                        _lib.check(fn(tr.h, key, which, buf.ctypes.data, n + 1, st), name)
                for which in (-1, 4):
                    with pytest.raises(_lib.EtudeHipError, match="etd_btrain: null argument or unknown buffer"):
                        _lib.check(fn(tr.h, key, which, buf.ctypes.data, n, st), name)
                with pytest.raises(_lib.EtudeHipError, match="etd_btrain: null argument or unknown buffer"):
                    _lib.check(fn(tr.h, key, 0, None, n, st), name)
                with pytest.raises(_lib.EtudeHipError, match="etd_btrain: null argument or unknown buffer"):
                    _lib.check(fn(None, key, 0, buf.ctypes.data, n, st), name)
        assert np.array_equal(tr.state_dict()[key.decode()], mini["state"][key.decode()])      # a refused write changed nothing
        assert all(not v.any() for v in tr.grads().values())
    finally:
        tr.close()


def test_checkpoint_round_trip_continues_bit_for_bit(mini):
    """two optimizer steps, then a second trainer from state_dict() and optimizer_state_dict(): one more step on the same batch gives the same bits in both"""
    from etude_amd import _lib
    cfg, batch = mini["cfg"], args_of(mini["batch"])
    a = trainer(cfg, mini["state"], 18)
    b = None
    try:
        for _ in range(2):
            a.loss_and_backward(*batch)
            a.step()
        sd, osd = a.state_dict(), a.optimizer_state_dict()
        assert osd["step"] == 2 and list(osd["exp_avg"]) == list(sd) and osd["exp_avg_sq"]["Transformer_layers.instr_attention_3.linear1.weight"].any()
        b = trainer(cfg, sd, 18)
        b.load_optimizer_state_dict(osd)
        assert b.global_step == 2 and _lib.lib().etd_btrain_get_step(b.h) == 2
        out = []
        for tr in (a, b):
            loss = tr.loss_and_backward(*batch)[0]
            g = tr.grads()
            norm = tr.step()
            out.append(dict(loss=np.float32(loss).tobytes(), norm=np.float64(norm).tobytes(), step=tr.global_step, g=g, p=tr.state_dict(), zg=tr.grads(),
                            o=tr.optimizer_state_dict()))
        x, y = out
        assert x["loss"] == y["loss"] and x["norm"] == y["norm"] and x["step"] == y["step"] == 3 and x["o"]["step"] == y["o"]["step"] == 3
        for k in sd:
            assert x["g"][k].tobytes() == y["g"][k].tobytes(), k
            assert x["p"][k].tobytes() == y["p"][k].tobytes(), k
            assert x["zg"][k].tobytes() == y["zg"][k].tobytes() and not x["zg"][k].any(), k
            for m in ("exp_avg", "exp_avg_sq"):
                assert x["o"][m][k].tobytes() == y["o"][m][k].tobytes(), (m, k)
        assert any(x["p"][k].tobytes() != sd[k].tobytes() for k in sd)      # the third step moved the parameters
    finally:
        a.close()
        if b is not None:
            b.close()
