"""Training of the EtudeDecoder on the device: the compute of the reference's ``train.py`` (:144-181).

``DecoderTrainer`` owns fp32 master weights, gradients and AdamW's two moments on the GPU (csrc/dec_train.hip, ``etd_dtrain_*``) and takes the batches
``EtudeDataset.collate_fn`` builds as they are::

    tr = DecoderTrainer(config, lr=2e-4, grad_accum_steps=4, lr_fn=lambda s: cosine_schedule_with_warmup(s, warmup, total))
    for batches in chunks_of(loader, 4):
        losses, norm = tr.train_step(batches)
    tr.save("latest.pth"); dec = tr.to_decoder(precision="f16")

Forward, backward of ``F.cross_entropy`` (labels not shifted, ignore index -100), gradient accumulation, ``clip_grad_norm_`` and ``torch.optim.AdamW`` are all HIP
kernels in fp32 -- the arithmetic of the reference on a CPU.  What is NOT matched: on CUDA the reference trains under fp16 autocast with a ``GradScaler``; there is no
mixed-precision mode here.  Dropout is 0 in the reference's configuration, so train mode computes what eval mode computes.  DESIGN.md 4j is the contract.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from pathlib import Path
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._trainer import Trainer
from .decoder import IGNORE_INDEX, EtudeDecoder, EtudeDecoderConfig, _int_array, expected_state_keys, right_padded_lengths

# the keys train.py:156-165 reads from a batch, with the C-ABI attribute order (the concat order of etude_decoder.py:171-176) for the four bin arrays
BATCH_ATTR_KEYS = ("pitch_overlap_bin_ids", "polyphony_bin_ids", "sustain_bin_ids", "rhythm_intensity_bin_ids")
BATCH_KEYS = ("input_ids", "attention_mask", "class_ids", "labels") + BATCH_ATTR_KEYS


def cosine_schedule_with_warmup(step: int, warmup: int, total: int, num_cycles: float = 0.5) -> float:
    """The lambda of ``transformers.get_cosine_schedule_with_warmup``: the factor the base learning rate is multiplied with at optimizer step ``step``."""
    if step < warmup:
        return float(step) / float(max(1, warmup))
    progress = float(step - warmup) / float(max(1, total - warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))


def state_shapes(cfg: EtudeDecoderConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """Shape of every tensor of the reference's state dict, in ``expected_state_keys`` order."""
    V, H, I, E, NB = cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.attribute_emb_dim, cfg.num_attribute_bins
    layer = {"input_layernorm.weight": (H,), "input_layernorm.bias": (H,), "post_attention_layernorm.weight": (H,), "post_attention_layernorm.bias": (H,),
             "attention.query_key_value.weight": (3 * H, H), "attention.query_key_value.bias": (3 * H,), "attention.dense.weight": (H, H),
             "attention.dense.bias": (H,), "mlp.dense_h_to_4h.weight": (I, H), "mlp.dense_h_to_4h.bias": (I,), "mlp.dense_4h_to_h.weight": (H, I),
             "mlp.dense_4h_to_h.bias": (H,)}
    fixed = {"word_embeddings.weight": (V, H), "class_embeddings.weight": (cfg.num_classes, H), "pitch_overlap_embeddings.weight": (NB, E),
             "polyphony_embeddings.weight": (NB, E), "note_sustain_embeddings.weight": (NB, E), "rhythm_intensity_embeddings.weight": (NB, E),
             "attribute_projection.weight": (H, 4 * E), "attribute_projection.bias": (H,), "transformer.embed_in.weight": (V, H),
             "transformer.final_layer_norm.weight": (H,), "transformer.final_layer_norm.bias": (H,), "lm_head.weight": (V, H)}
    out = OrderedDict()
    for k in expected_state_keys(cfg):
        out[k] = fixed[k] if k in fixed else layer[k.split(".", 3)[3]]
    return out


def init_decoder_state(cfg: EtudeDecoderConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """``EtudeDecoder._init_weights`` (etude_decoder.py:125-134): normal(0, initializer_range) for embeddings and linears, zero padding rows and biases, LayerNorm
    1 / 0.  The values come from numpy's generator: the distribution is the contract, not torch's stream."""
    rng = np.random.default_rng(seed)
    pads = {"word_embeddings.weight": cfg.pad_token_id, "class_embeddings.weight": cfg.pad_class_id, "transformer.embed_in.weight": cfg.pad_token_id}
    out = OrderedDict()
    for k, shape in state_shapes(cfg).items():
        if "layernorm" in k or "layer_norm" in k:
            out[k] = np.ones(shape, np.float32) if k.endswith(".weight") else np.zeros(shape, np.float32)
        elif k.endswith(".bias"):
            out[k] = np.zeros(shape, np.float32)
        else:
            w = (float(cfg.initializer_range) * rng.standard_normal(shape)).astype(np.float32)
            if k in pads:
                w[pads[k]] = 0
            elif k.endswith("_embeddings.weight"):
                w[cfg.attribute_pad_id] = 0
            out[k] = w
    return out


def check_train_config(cfg: EtudeDecoderConfig) -> None:
    """The limits of ``etd_dtrain_create``, as a ValueError before any GPU is needed."""
    H, nh = int(cfg.hidden_size), int(cfg.num_attention_heads)
    if nh < 1 or H != 64 * nh:
        raise ValueError(f"DecoderTrainer: head_dim must be 64 (hidden_size {H}, {nh} heads)")
    if int(64 * cfg.rotary_pct) != 16:
        raise ValueError(f"DecoderTrainer: 16 rotary dims only (rotary_pct {cfg.rotary_pct})")
    if H % 256:
        raise ValueError(f"DecoderTrainer: hidden_size {H} is not a multiple of 256")
    if int(cfg.intermediate_size) % 128:
        raise ValueError(f"DecoderTrainer: intermediate_size {cfg.intermediate_size} is not a multiple of 128")
    for name in ("vocab_size", "num_classes", "num_attribute_bins", "attribute_emb_dim", "max_position_embeddings"):
        if int(getattr(cfg, name)) < 1:
            raise ValueError(f"DecoderTrainer: {name} must be positive")
    if int(cfg.num_hidden_layers) < 0:
        raise ValueError("DecoderTrainer: num_hidden_layers must not be negative")


def pack_batch(cfg: EtudeDecoderConfig, batch: Dict[str, object]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """A ``collate_fn`` batch (torch or numpy, [B, T]) -> the packed ragged rows the engine takes: ``(T [n], ids [M], cls [M], attrs4 [4][M], labels [M])``, int32.
    ValueError for a missing key, mismatched shapes, left padding or holes, a label on a padded position, ids / classes / bins / labels outside their tables,
    and a sequence longer than ``max_position_embeddings``.  Rows of no valid position are dropped."""
    missing = [k for k in BATCH_KEYS if k not in batch]
    if missing:
        raise ValueError(f"batch lacks {missing} (the keys train.py reads: {list(BATCH_KEYS)})")
    ids = _int_array(batch["input_ids"], "input_ids")
    if ids.ndim != 2:
        raise ValueError(f"input_ids must be [batch, seq_len], got shape {ids.shape}")
    B, T = ids.shape
    lab = _int_array(batch["labels"], "labels")
    lens = right_padded_lengths((B, T), batch["attention_mask"], lab)
    if lens.size and int(lens.max()) > int(cfg.max_position_embeddings):
        raise ValueError(f"a sequence of {int(lens.max())} positions, max_position_embeddings is {cfg.max_position_embeddings}")
    valid = np.arange(T)[None, :] < lens[:, None]
    cols = []
    for name, hi in (("class_ids", cfg.num_classes),) + tuple((k, cfg.num_attribute_bins) for k in BATCH_ATTR_KEYS):
        a = _int_array(batch[name], name)
        if a.shape != (B, T):
            raise ValueError(f"{name} of shape {a.shape}, input_ids {(B, T)}")
        a = a[valid]
        if a.size and (a.min() < 0 or a.max() >= hi):
            raise ValueError(f"{name} holds a value outside [0, {hi})")
        cols.append(a)
    pid = ids[valid]
    if pid.size and (pid.min() < 0 or pid.max() >= cfg.vocab_size):
        raise ValueError(f"input_ids holds a value outside [0, {cfg.vocab_size})")
    pl = lab[valid]
    scored = pl[pl != IGNORE_INDEX]
    if scored.size and (scored.min() < 0 or scored.max() >= cfg.vocab_size):
        raise ValueError(f"labels holds a value outside [0, {cfg.vocab_size}) that is not {IGNORE_INDEX}")
    i32 = lambda a: np.ascontiguousarray(a, np.int32)      # noqa: E731
    return i32(lens[lens > 0]), i32(pid), i32(cols[0]), i32(np.stack(cols[1:])), i32(pl)


class DecoderTrainer(Trainer):
    """fp32 training of the EtudeDecoder on the GPU.  ``state=None`` initialises as the reference does (``init_decoder_state(config, seed)``); otherwise ``state`` maps
    the reference's state-dict keys to arrays.  ``lr_fn(step)`` is the factor on ``lr`` at optimizer step ``step`` (None = 1; ``cosine_schedule_with_warmup``).
    ``max_rows`` bounds the valid positions of one batch and sizes the activation workspace (default: 8 full-length sequences)."""
    _destroy = "etd_dtrain_destroy"
    _abi = "etd_dtrain"

    def __init__(self, config: EtudeDecoderConfig, state: Optional[Dict[str, np.ndarray]] = None, seed: int = 0, device: Union[str, torch.device] = "cuda",
                 lr: float = 2e-4, betas: Tuple[float, float] = (0.9, 0.98), eps: float = 1e-8, weight_decay: float = 0.01, clip_grad_norm: float = 1.0,
                 grad_accum_steps: int = 4, lr_fn: Optional[Callable[[int], float]] = None, max_rows: Optional[int] = None):
        check_train_config(config)
        if int(grad_accum_steps) < 1:
            raise ValueError("grad_accum_steps must be at least 1")
        self.config = config
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.clip_grad_norm, self.grad_accum_steps, self.lr_fn = float(clip_grad_norm), int(grad_accum_steps), lr_fn
        self.max_rows = int(max_rows) if max_rows else 8 * int(config.max_position_embeddings)
        self._shapes = state_shapes(config)
        if state is None:
            state = init_decoder_state(config, seed)
        else:
            for k, shape in self._shapes.items():
                if k not in state:
                    raise ValueError(f"state lacks '{k}'")
                if tuple(np.shape(state[k])) != shape:
                    raise ValueError(f"state['{k}'] has shape {tuple(np.shape(state[k]))}, expected {shape}")
        if device == "auto":
            device = "cuda"
        self.device = torch.device(device)
        self._device()
        cfg = _lib.DecCfg(vocab_size=config.vocab_size, hidden_size=config.hidden_size, num_hidden_layers=config.num_hidden_layers,
                          num_attention_heads=config.num_attention_heads, intermediate_size=config.intermediate_size,
                          max_position_embeddings=config.max_position_embeddings, num_classes=config.num_classes,
                          num_attribute_bins=config.num_attribute_bins, attribute_emb_dim=config.attribute_emb_dim, rotary_pct=config.rotary_pct,
                          rope_theta=config.rope_theta, layer_norm_eps=config.layer_norm_eps, max_streams=1, max_ctx=config.max_position_embeddings,
                          precision=0, max_prefill_rows=0)
        names, ptrs, numels, n, keep = _lib.weights_arrays({k: state[k] for k in self._shapes})
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().etd_dtrain_create(C.byref(cfg), names, ptrs, numels, n, int(config.pad_token_id), int(config.pad_class_id),
                                                    int(config.attribute_pad_id), self.max_rows, C.byref(h)), "etd_dtrain_create")
        del keep
        self._adopt(h)
        self._ts = torch.cuda.Stream(device=self.device)
        self.global_step = 0          # optimizer steps taken: the schedule's argument
        self._micro = 0               # batches since the last step (skipped ones included, as train.py counts batch_idx)

    # ------------------------------------------------------------------ plumbing
    def _stream(self, dev=None):
        """the trainer's own stream, not the current one"""
        return C.c_void_p(self._ts.cuda_stream)

    def _read_entry(self, which: int):
        return (("read_param", ()), ("read_grad", ()), ("read_moment", (0,)), ("read_moment", (1,)))[which]

    # ------------------------------------------------------------------ one batch
    def loss_and_backward(self, batch: Dict[str, object]) -> Tuple[float, int, bool]:
        """Forward and backward of one ``collate_fn`` batch: ``(loss, n_scored, skipped)``.  ``1 / grad_accum_steps`` times the gradient of the loss is added to the
        accumulated gradients.  A batch with no label but -100 has loss nan, is skipped and changes no bit of them."""
        return self.packed_loss_and_backward(*pack_batch(self.config, batch))

    def packed_loss_and_backward(self, T, ids, cls, attrs4, labels) -> Tuple[float, int, bool]:
        self._micro += 1
        if T.size == 0:
            return float("nan"), 0, True
        loss, n_scored = C.c_float(), C.c_int32()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().etd_dtrain_forward_backward(self.h, int(T.size), T.ctypes.data, ids.ctypes.data, cls.ctypes.data, attrs4.ctypes.data,
                                                              labels.ctypes.data, 1.0 / self.grad_accum_steps, C.byref(loss), C.byref(n_scored), self._stream()),
                       "etd_dtrain_forward_backward")
        return float(loss.value), int(n_scored.value), n_scored.value == 0

    def current_lr(self) -> float:
        return self.lr * (float(self.lr_fn(self.global_step)) if self.lr_fn is not None else 1.0)

    def _step_call(self, norm_ref, stream) -> None:
        self._call("clip_and_step", self.clip_grad_norm, self.current_lr(), self.betas[0], self.betas[1], self.eps, self.weight_decay, norm_ref, stream)

    def step(self) -> float:
        """``clip_grad_norm_`` + ``AdamW.step`` + ``scheduler.step`` + ``zero_grad`` (train.py:175-181).  Returns the gradient norm before clipping."""
        norm = super().step()
        self._micro = 0
        return norm

    def train_step(self, batches: Sequence[Dict[str, object]]) -> Tuple[List[float], float]:
        """``grad_accum_steps`` batches, then one optimizer step: ``(the batches' losses, gradient norm before clipping)``."""
        if len(batches) != self.grad_accum_steps:
            raise ValueError(f"train_step takes grad_accum_steps = {self.grad_accum_steps} batches, got {len(batches)}")
        losses = [self.loss_and_backward(b)[0] for b in batches]
        return losses, self.step()

    # ------------------------------------------------------------------ state (state_dict, grads and the optimizer's state: Trainer)
    def workspace_bytes(self) -> int:
        return int(_lib.lib().etd_dtrain_bytes(self.h, 0))

    def save(self, path: Union[str, Path]) -> None:
        """The training payload ``{"model_state_dict": ...}`` that ``load_decoder_state`` / ``load_etude_decoder`` read back."""
        torch.save({"model_state_dict": OrderedDict((k, torch.from_numpy(v)) for k, v in self.state_dict().items()), "global_step": self.global_step}, str(path))

    def to_decoder(self, precision: Optional[str] = None, **kwargs) -> EtudeDecoder:
        """An inference ``EtudeDecoder`` over a copy of the current weights."""
        return EtudeDecoder(self.config, self.state_dict(), device=self.device, precision=precision, **kwargs)
