"""From audio to scores: ``evaluate_separator`` runs a ``StemSeparator`` on the mixes of a test set and hands the estimated stems, where they lie on the device, to
``BSSEval``.  ``validate()`` and ``fit()`` of etude_amd.separator_data are the training loop's loss and are not involved."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .bss import METRICS, BSSEval, BSSEvalConfig, aggregate


def _audio(x, what: str, rate: int, channels: int, sample_rate: Optional[int]):
    """a path (read as WAV) or an array / tensor [channels][N] at ``sample_rate`` (None: the separator's) -> the samples, after the rate and channel checks"""
    sr = rate if sample_rate is None else int(sample_rate)
    if isinstance(x, (str, Path)):
        from .extractor import read_wav
        x, sr = read_wav(x)
    if sr != rate:
        raise ValueError(f"{what}: sampled at {sr} Hz, the separator's config says {rate}")
    shp = tuple(x.shape) if hasattr(x, "shape") else None
    if shp is None or len(shp) != 2 or shp[0] != channels:
        raise ValueError(f"{what}: need [{channels}][N] samples (the separator's n_channels), got shape {shp}")
    return x


def evaluate_separator(separator, tracks: Sequence, bss: Optional[BSSEval] = None, instruments: Optional[Sequence[str]] = None,
                       sample_rate: Optional[int] = None) -> Dict:
    """tracks: ``(mix_wav, stem_wavs)`` pairs; ``mix_wav`` a WAV path or [channels][N] samples, ``stem_wavs`` a dict instrument -> path or samples of the same
    length.  ``instruments``: the ones to score (default: all of the separator's config, in its order).  ``sample_rate``: the rate of samples given as arrays
    (default: the config's); a rate or channel count other than the separator's config is refused.  ``bss``: a ``BSSEval`` (default: 512 taps, windows and hop of
    one second at the config's rate).

    -> ``{"tracks": [{instrument: {metric: track score}}], "aggregate": {instrument: {metric: corpus score}}, "n_tracks", "n_skipped", "results"}``;
    ``results`` is ``BSSEval.evaluate_many``'s list.  The estimates go from ``separate_many`` to ``BSSEval`` on the device, with no host copy."""
    cfg = separator.config
    names = list(instruments) if instruments is not None else list(cfg.instruments)
    unknown = [n for n in names if n not in cfg.instruments]
    if unknown or not names:
        raise ValueError(f"evaluate_separator: instruments {unknown or names} are not among the separator's {cfg.instruments}")
    index = [cfg.instruments.index(n) for n in names]
    if bss is None:
        bss = BSSEval(BSSEvalConfig(window=cfg.sample_rate, hop=cfg.sample_rate), device=separator.device)
    mixes, refs = [], []
    for i, (mix, stems) in enumerate(tracks):
        mix = _audio(mix, f"track {i}: the mix", cfg.sample_rate, cfg.n_channels, sample_rate)
        missing = [n for n in names if n not in stems]
        if missing:
            raise ValueError(f"track {i}: no stem for {missing}")
        ref = [_audio(stems[n], f"track {i}: stem {n!r}", cfg.sample_rate, cfg.n_channels, sample_rate) for n in names]
        if any(tuple(r.shape) != tuple(mix.shape) for r in ref):
            raise ValueError(f"track {i}: the stems' shapes {[tuple(r.shape) for r in ref]} differ from the mix's {tuple(mix.shape)}")
        mixes.append(mix)
        refs.append(ref)
    dev = separator._device()
    ests = separator.separate_many(mixes)
    if index != list(range(len(cfg.instruments))):
        sel = torch.as_tensor(index, device=dev)
        ests = [e.index_select(0, sel) for e in ests]
    refs_dev = [torch.stack([torch.as_tensor(r).to(dev, torch.float32) for r in ref]) for ref in refs]
    results = bss.evaluate_many(refs_dev, ests)
    agg = aggregate(results)
    return dict(tracks=[{n: {k: float(r["scores"][k][j]) for k in METRICS} for j, n in enumerate(names)} for r in results],
                aggregate={n: {k: float(agg[k][j]) for k in METRICS} for j, n in enumerate(names)} if results else {},
                n_tracks=agg["n_tracks"], n_skipped=agg["n_skipped"], results=results)
