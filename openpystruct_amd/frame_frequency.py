"""A natural-frequency floor in multi-load-case frame design sizing.

The design objective of `optimize_frame_designs` / `optimize_grouped_frame_designs` with one more term:

    L(I)  = sum_e I_e + agg_c P_c(I) + P_f(I)             P_f = alpha * sum_{j < m} h_j^2,   h_j = max(0, 1 - lambda_j(I) / floor)
    dP_f/dI_e = sum_{j < m} (-2 alpha h_j / floor) phi_j,e . (K_b,e phi_j,e)                  floor = (2 pi f_min)^2

lambda_j the m lowest eigenvalues of K(I) phi = lambda M phi (`frame_modes`).  All m tracked modes are hinged against the same floor:
the term is a symmetric function of the tracked cluster and stays differentiable where the two lowest modes cross.  It is
dimensionless, and like the sway term it is a PENALTY, not a constraint: with a finite alpha the floor is approached, not met.
Under aggregate="max" it is added after the max; it is not one of the cases.

M does not depend on I, so the gradient is one streaming launch (ops_frame_frequency_floor_f64, csrc/frame_loads.hip) and no adjoint
solve; the eigenpairs come from the subspace iteration of `frame_modes`, continued across the epochs of a loop on each epoch's new
factor from the R = M Q the last Ritz step left -- no restart.  The design and group steps take the term through the two arrays of
their *_dyn entries (include/openpystruct_amd_frame_frequency.h), which are not specific to frequency.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _cabi
from .frame_modes import MAX_VECTORS, FrameMass, FrameModes, _ModeIteration, default_vectors
from .frames import FrameFactor, FrameTopology, _adjoint_tables


class FrequencyFloor:
    """The term `frequency=` of the design entries: the first `n_modes` natural frequencies of every design are held above
    `min_frequency` (Hz; a scalar, or [G]: one per design) by the penalty alpha * sum_j max(0, 1 - lambda_j / floor)^2.

    `mass`: the `FrameMass` of the topology being sized.  `n_vectors` (default: that of `frame_modes`), `X0`: the subspace and its
    start, as in `frame_modes`; 1 <= n_modes <= n_vectors <= min(8, n_eq).  `start_iters`: the iterations of the cold start, in the
    first epoch of a loop and in `evaluate_frame_designs` / the gradient entries; `iters` >= 1: the iterations of every later epoch,
    which continue the iteration of the epoch before on the new factor.  The eigenpairs of an epoch are therefore those of a
    TRUNCATED iteration, and the gradient is the gradient of the penalty at those pairs: `.modes.change`, the epoch-to-epoch
    relative change of the Ritz values, is the thing to look at when choosing `iters` (DESIGN.md §9r has measured deviations).

    The object owns the iteration's buffers, keyed by (G, n_vectors); a loop allocates nothing and reads nothing back beyond its
    `poll_every`.  After a run: `.modes`, a `FrameModes` of the last solve's inertias (eigenvalues, frequencies, shapes, change,
    status) and `.penalty` [G] float64 (with a `catalogue=`, those of the last evaluation: the continuous design's).  A design whose
    mode status becomes non-zero (its factorisation failed, or X^T M X lost positive definiteness: `frame_modes`) gets a NaN
    gradient and a NaN loss, exactly as a design with a failed factorisation does.  Limits: those of `frame_factor` and
    `frame_modes`, half bandwidth <= 55 and n_vectors <= 8."""

    def __init__(self, mass: FrameMass, min_frequency, alpha: float = 1.0, n_modes: int = 2, n_vectors: Optional[int] = None,
                 iters: int = 2, start_iters: int = 16, X0: Optional[torch.Tensor] = None):
        if not isinstance(mass, FrameMass):
            raise ValueError("mass must be a FrameMass")
        topo = mass.topo
        f = np.asarray(min_frequency.detach().cpu().numpy() if torch.is_tensor(min_frequency) else min_frequency, dtype=np.float64)
        if f.ndim > 1 or f.size < 1 or not np.all(np.isfinite(f)) or not np.all(f > 0.0):
            raise ValueError("min_frequency must be a scalar or [G], finite and > 0 (Hz)")
        if not float(alpha) >= 0.0 or not math.isfinite(float(alpha)):
            raise ValueError("alpha must be finite and >= 0")
        m = int(n_modes)
        p = default_vectors(topo, m) if n_vectors is None else int(n_vectors)
        if m < 1 or not m <= p <= min(MAX_VECTORS, topo.n_eq):
            raise ValueError(f"1 <= n_modes <= n_vectors <= min({MAX_VECTORS}, n_eq = {topo.n_eq}) needed, got n_modes = {m}, n_vectors = {p}")
        if int(iters) < 1 or int(start_iters) < 1:
            raise ValueError("iters >= 1 and start_iters >= 1 needed")
        if X0 is not None and not (torch.is_tensor(X0) and X0.dtype == torch.float64 and X0.dim() in (3, 4)
                                   and tuple(X0.shape[-3:]) == (p, topo.Nn, 3)):
            raise ValueError(f"X0 must be float64 [{p}, {topo.Nn}, 3] or [G, {p}, {topo.Nn}, 3]")
        self.mass, self.topo, self.alpha, self.n_modes, self.n_vectors = mass, topo, float(alpha), m, p
        self.iters, self.start_iters, self.X0 = int(iters), int(start_iters), X0
        self.min_frequency = f
        self.floor = (2.0 * math.pi * f) ** 2
        self.modes: Optional[FrameModes] = None
        self.penalty: Optional[torch.Tensor] = None
        self._buffers, self._bound = {}, None

    # ---- checks: all before any device call ----
    def check(self, topo: FrameTopology, G: int) -> None:
        """The term against the problem of an entry: the topology, the batch of a per-frame nodal mass, of `min_frequency` and of X0."""
        if self.mass.topo is not topo:
            raise ValueError("mass must be a FrameMass of this topology")
        if self.mass.batch is not None and self.mass.batch != G:
            raise ValueError(f"nodal_mass is per frame for {self.mass.batch} frames, the factor holds {G}")
        if self.floor.ndim == 1 and self.floor.shape[0] != G:
            raise ValueError(f"min_frequency is per design for {self.floor.shape[0]} designs, there are {G}")
        if self.X0 is not None and self.X0.dim() == 4 and self.X0.shape[0] != G:
            raise ValueError(f"X0 must be float64 [{self.n_vectors}, {topo.Nn}, 3] or [{G}, {self.n_vectors}, {topo.Nn}, 3]")

    # ---- buffers ----
    def _buffer(self, name: str, shape: tuple, dtype=torch.float64) -> torch.Tensor:
        key = (name, shape, self._dev)
        t = self._buffers.get(key)
        if t is None:
            t = self._buffers[key] = torch.empty(shape, dtype=dtype, device=self._dev)
        return t

    def bind(self, G: int, dev, iteration: bool = True) -> None:
        """Everything a run of G designs on `dev` needs, allocated (or found, by shape) here: the iteration's buffers, the floor, the
        two arrays the step reads."""
        if self.mass.d_mass.device != dev or (self.X0 is not None and self.X0.device != dev):
            raise ValueError(f"the mass tables and X0 must be on {dev}, where the designs are")
        self._dev = dev
        self._it = _ModeIteration(self.topo, self.mass, G, self.n_vectors, self._buffer) if iteration else None
        self.grad_extra, self._penalty = self._buffer("grad_extra", (G, self.topo.Ne)), self._buffer("penalty", (G,))
        key = ("floor", dev)
        if key not in self._buffers:
            self._buffers[key] = torch.as_tensor(np.atleast_1d(self.floor), dtype=torch.float64, device=dev)
        self._floor = self._buffers[key]
        self._bound = G

    @property
    def extras(self) -> tuple:
        """(grad_extra [G,Ne], penalty_extra [G]): what the *_dyn step entries are given."""
        return self.grad_extra, self._penalty

    # ---- launches on the current stream ----
    def start(self) -> None:
        self._it.start(self.X0)

    def advance(self, factor: FrameFactor) -> None:
        """`start_iters` iterations after a start, `iters` after that, on `factor`."""
        self._it.advance(factor, self.start_iters if self._it.n_run == 0 else self.iters)

    def floor_launch(self, active: Optional[torch.Tensor], phi: Optional[torch.Tensor] = None, lam: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None, p: Optional[int] = None) -> None:
        """ops_frame_frequency_floor_f64 into `extras`, from the iteration's Q, lambda and status or from the caller's."""
        topo, G, it = self.topo, self._bound, self._it
        if phi is None:
            phi, lam, status, p = it.Q, it.lam, it.status, self.n_vectors
        with torch.cuda.device(self._dev):
            rc = _cabi.load().ops_frame_frequency_floor_f64(
                G, self.n_modes, p, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), _adjoint_tables(topo).conn.data_ptr(),
                phi.data_ptr(), lam.data_ptr(), status.data_ptr(), self._floor.data_ptr(), int(self._floor.numel() > 1), self.alpha,
                None if active is None else active.data_ptr(), self.grad_extra.data_ptr(), self._penalty.data_ptr(),
                torch.cuda.current_stream(self._dev).cuda_stream)
        _cabi.check(rc, "ops_frame_frequency_floor_f64")

    def cold(self, factor: FrameFactor) -> None:
        """A cold iteration of `start_iters` on `factor` and the floor kernel for every design."""
        self.start()
        self.advance(factor)
        self.floor_launch(None)

    def finish(self) -> None:
        """`.modes` and `.penalty` as new tensors, from the iteration's state."""
        self.modes = self._it.result(self.n_modes)
        self.penalty = self._penalty.clone()

    def from_modes(self, modes: FrameModes, G: int, dev) -> None:
        """The floor kernel on a caller's `FrameModes` (at least n_modes of them), no iteration."""
        topo, m = self.topo, self.n_modes
        sh, lam, st = modes.shapes, modes.eigenvalues, modes.status
        if not (torch.is_tensor(sh) and sh.dtype == torch.float64 and sh.dim() == 4 and sh.shape[0] == G and m <= sh.shape[1] <= MAX_VECTORS
                and tuple(sh.shape[2:]) == (topo.Nn, 3)):
            raise ValueError(f"modes.shapes must be float64 [{G}, m, {topo.Nn}, 3] with {m} <= m <= {MAX_VECTORS}")
        if not (torch.is_tensor(lam) and lam.dtype == torch.float64 and tuple(lam.shape) == tuple(sh.shape[:2])):
            raise ValueError(f"modes.eigenvalues must be float64 [{G}, {sh.shape[1]}]")
        if not (torch.is_tensor(st) and st.dtype == torch.int32 and tuple(st.shape) == (G,)):
            raise ValueError(f"modes.status must be int32 [{G}]")
        if not (sh.is_cuda and lam.is_cuda and st.is_cuda):
            raise RuntimeError("frequency= needs GPU tensors: openpystruct_amd has no CPU fallback")
        self.bind(G, dev, iteration=False)
        self.floor_launch(None, sh.contiguous(), lam.contiguous(), st.contiguous(), int(sh.shape[1]))
