"""The separator's multichannel Wiener stage, restated with torch-CPU ops in a dtype of the caller's choice: ``torch.float64`` is the truth,
``torch.float32`` the yardstick the device stage's error is measured against (the device does the algebra in fp64 and rounds Y to fp32 once per iteration; that
rounding is part of its measured error, the restatement keeps Y in its dtype).

Modelled on norbert.wiener / expectation_maximization; the contract is this project's own and parity with norbert is unpinned.  X [C][Tf][F] complex is the
mixture below bin F, Y [I][C][Tf][F] the masked spectra (the ratio mask is the initial estimate), C = 1 or 2."""
from __future__ import annotations

import torch

EPS = 2.0 ** -23
CHUNK = 64                # frames per partial sum of the source model


def _cdtype(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def song_scale(X: torch.Tensor, dtype) -> torch.Tensor:
    """s = max(1, max|X| / 10) over every channel, frame and bin"""
    X = X.to(_cdtype(dtype))
    return torch.clamp(X.abs().max() / 10, min=1.0).to(dtype)


def chunked_sum(a: torch.Tensor) -> torch.Tensor:
    """the sum over dim -2 (frames): partial sums over consecutive chunks of 64 frames, the chunks added in ascending order"""
    Tf = a.shape[-2]
    tot = torch.zeros(a.shape[:-2] + a.shape[-1:], dtype=a.dtype)
    for t0 in range(0, Tf, CHUNK):
        tot = tot + a[..., t0:t0 + CHUNK, :].sum(-2)
    return tot


def source_model(y: torch.Tensor):
    """y [I][C][Tf][F] (already over s) -> v [I][Tf][F] = (1 / C) sum_c |y|^2 and R [I][C][C][F] = sum_t y y^H / (eps + sum_t v)"""
    C = y.shape[1]
    v = (y.real ** 2 + y.imag ** 2).sum(1) / C
    num = chunked_sum(y[:, :, None] * y.conj()[:, None, :])
    den = EPS + chunked_sum(v)
    return v, num / den[:, None, None]


def inverse(Cxx: torch.Tensor) -> torch.Tensor:
    """the closed-form inverse of [C][C][...]: 1 / Cxx for C = 1, the adjugate over a d - b c for C = 2"""
    if Cxx.shape[0] == 1:
        return 1.0 / Cxx
    (a, b), (c, d) = Cxx
    det = a * d - b * c
    return torch.stack([torch.stack([d, -b]), torch.stack([-c, a])]) / det


def iteration(X: torch.Tensor, Y: torch.Tensor, s: torch.Tensor, dtype, parts=None) -> torch.Tensor:
    """one pass: source model, mixture model Cxx = sum_j v_j R_j + reg I, y_j <- v_j R_j Cxx^-1 x on y / s and x / s, times s.  ``parts`` (a dict) collects
    v, R, Cxx and z = Cxx^-1 (x / s)"""
    cd = _cdtype(dtype)
    C = X.shape[0]
    if C not in (1, 2) or Y.shape[1] != C:
        raise ValueError(f"multichannel Wiener filtering takes 1 or 2 channels, got X {tuple(X.shape)}, Y {tuple(Y.shape)}")
    x, y = X.to(cd) / s, Y.to(cd) / s
    reg = torch.tensor(EPS, dtype=dtype).sqrt()
    v, R = source_model(y)
    Cxx = (v[:, None, None] * R[:, :, :, None, :]).sum(0) + (reg * torch.eye(C, dtype=dtype))[:, :, None, None]
    z = torch.einsum("cdtk,dtk->ctk", inverse(Cxx), x)
    if parts is not None:
        parts.update(v=v, R=R, Cxx=Cxx, z=z, reg=reg)
    return v[:, None] * torch.einsum("jcdk,dtk->jctk", R, z) * s


def wiener(X: torch.Tensor, Y: torch.Tensor, iterations: int, dtype, scale=None) -> torch.Tensor:
    """``iterations`` passes (0 .. 8; 0 returns Y untouched) -> Y [I][C][Tf][F].  ``scale`` forces s, for a test to show what a wrong s would give"""
    if int(iterations) != iterations or not 0 <= iterations <= 8:
        raise ValueError(f"mwf_iterations must be an integer in 0 .. 8, got {iterations}")
    Y = Y.to(_cdtype(dtype))
    s = song_scale(X, dtype) if scale is None else torch.tensor(float(scale), dtype=dtype)
    for _ in range(int(iterations)):
        Y = iteration(X, Y, s, dtype)
    return Y
