"""Natural frequencies and mode shapes of batched 2-D frames on the kept factorisation.

The generalised eigenproblem is K(I) phi = lambda M phi on the free DOFs, K the matrix `frame_factor` factorises and M the sum of
the element mass (a mass per unit length: the consistent 6 x 6 matrix, or lumped, m L / 2 on the four translations of an element)
and nodal masses.  M does not depend on I.  The lowest modes come from a subspace (inverse) iteration with a Rayleigh-Ritz step:
per iteration the re-solve of `frame_resolve` with the right-hand sides M Q, the mass apply and the Ritz step of
csrc/frame_loads.hip (arithmetic: csrc/frame_modes.hpp) -- three launches, no factorisation, no CPU path.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _cabi
from .frames import FrameCaseSolution, FrameFactor, FrameTopology, _adjoint_tables, _checked, _resolve_launch, frame_factor

MAX_VECTORS = 8          # csrc/frame_modes.hpp FM_MAX_VECTORS
KINDS = ("consistent", "lumped")


class FrameMass:
    """The mass of a frame, checked and on the topology's device: `mass_per_length` (kg/m) a scalar or [Ne], strictly positive;
    `nodal_mass` [Nn,3] (shared by the batch) or [B,Nn,3] (per frame), >= 0, the mass on (ux, uy, rz) of every node, None = none;
    `kind`: "consistent" (the standard 6 x 6 matrix of a prismatic beam, rotated as the stiffness is) or "lumped" (m L / 2 on the
    four translational end DOFs and nothing on the rotations: what OpenSees does for `-mass` without `-cMass`)."""

    def __init__(self, topo: FrameTopology, mass_per_length, nodal_mass=None, kind: str = "consistent"):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}")
        to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)  # noqa: E731
        m = np.asarray(to_np(mass_per_length), dtype=np.float64)
        if m.shape not in ((), (topo.Ne,)) or not np.all(np.isfinite(m)) or not np.all(m > 0.0):
            raise ValueError(f"mass_per_length must be a scalar or [{topo.Ne}], finite and strictly positive")
        self.topo, self.kind, self.consistent = topo, kind, int(kind == "consistent")
        self.mass_per_length = np.broadcast_to(m, (topo.Ne,)).copy()
        self.d_mass = torch.tensor(self.mass_per_length, dtype=torch.float64, device=topo.device)
        self.nodal_mass, self.d_nodal, self.batch = None, None, None
        if nodal_mass is not None:
            nm = np.asarray(to_np(nodal_mass), dtype=np.float64)
            if nm.ndim not in (2, 3) or nm.shape[-2:] != (topo.Nn, 3) or not np.all(np.isfinite(nm)) or not np.all(nm >= 0.0):
                raise ValueError(f"nodal_mass must be [{topo.Nn}, 3] or [B, {topo.Nn}, 3], finite and >= 0")
            self.nodal_mass = nm
            self.d_nodal = torch.tensor(nm, dtype=torch.float64, device=topo.device)
            self.batch = nm.shape[0] if nm.ndim == 3 else None

    @property
    def nodal_bstride(self) -> int:
        return 3 * self.topo.Nn if self.batch is not None else 0


class FrameModes(NamedTuple):
    eigenvalues: torch.Tensor    # [B, m]        lambda = omega^2, ascending
    frequencies: torch.Tensor    # [B, m]        Hz: sqrt(lambda) / (2 pi)
    shapes: torch.Tensor         # [B, m, Nn, 3] phi^T M phi = 1; the component of largest magnitude is positive
    change: torch.Tensor         # [B, m]        |lambda - lambda of the iteration before| / lambda
    iterations: int
    status: torch.Tensor         # [B] int32     0; 1: the factorisation or a re-solve failed; 2: X^T M X not positive definite


def default_vectors(topo: FrameTopology, n_modes: int) -> int:
    return min(MAX_VECTORS, topo.n_eq, max(2 * n_modes, n_modes + 4))


def default_start(topo: FrameTopology, p: int) -> np.ndarray:
    """X0[j,n,d] = 1 + cos(0.37 (j + 1) (3 n + d + 1)), zero on constrained DOFs: float64 [p,Nn,3] (numpy)."""
    k = np.arange(3 * topo.Nn, dtype=np.float64).reshape(topo.Nn, 3) + 1.0
    x0 = 1.0 + np.cos(0.37 * (np.arange(p, dtype=np.float64)[:, None, None] + 1.0) * k[None])
    return np.where(topo.fix3[None], 0.0, x0)


def _free_mask(topo: FrameTopology) -> torch.Tensor:
    t = topo.__dict__.get("_free_mask")
    if t is None:
        t = topo.__dict__["_free_mask"] = torch.as_tensor((~topo.fix3).astype(np.float64), device=topo.device)
    return t


def _mass_apply(mass: FrameMass, rows: int, rows_per_frame: int, x: torch.Tensor, y: torch.Tensor) -> None:
    """ops_frame_mass_apply_f64 on the current stream: y[r] = M x[r] for `rows` rows [Nn,3]."""
    topo = mass.topo
    adj = _adjoint_tables(topo)
    dev = x.device
    with torch.cuda.device(dev):
        rc = _cabi.load().ops_frame_mass_apply_f64(
            rows, rows_per_frame, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), adj.conn.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(),
            mass.d_mass.data_ptr(), mass.consistent, None if mass.d_nodal is None else mass.d_nodal.data_ptr(), mass.nodal_bstride,
            x.data_ptr(), y.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_frame_mass_apply_f64")


class _ModeIteration:
    """The subspace iteration of B frames on p vectors: its buffers (from `buffer(name, shape[, dtype])`, which keeps them by shape),
    its start and `advance`.  After an advance `Q` [B,p,Nn,3] holds the M-normalised Ritz vectors, `lam` and `change` [B,p] the Ritz
    values and their relative change against the values `lam` held before, `status` [B] the frames' status, and `R` = M Q: the next
    advance -- on this factor or on another one of the same frames -- continues from it with no restart launch."""

    def __init__(self, topo: FrameTopology, mass: FrameMass, B: int, p: int, buffer):
        self.topo, self.mass, self.B, self.p = topo, mass, B, p
        shape = self.shape = (B, p, topo.Nn, 3)
        self.out = FrameCaseSolution(buffer("modes_X", shape), buffer("modes_forces", (B, p, topo.Ne, 6)), buffer("modes_V", (B, p, topo.Ne)),
                                     buffer("modes_M", (B, p, topo.Ne)), buffer("modes_row_status", (B, p), torch.int32))
        self.X, self.MX, self.R, self.Q = self.out.disp, buffer("modes_MX", shape), buffer("modes_R", shape), buffer("modes_Q", shape)
        self.lam, self.change, self.status = buffer("modes_lambda", (B, p)), buffer("modes_change", (B, p)), buffer("modes_status", (B,), torch.int32)
        self.n_run = 0

    def start(self, X0: Optional[torch.Tensor] = None) -> None:
        """R = M X0 (`default_start` without X0; the values on constrained DOFs zeroed), lambda = +inf: two launches and a fill."""
        topo, p = self.topo, self.p
        if X0 is None:
            x0 = topo.__dict__.setdefault("_modes_x0", {}).get(p)
            if x0 is None:
                x0 = topo.__dict__["_modes_x0"][p] = torch.as_tensor(default_start(topo, p), dtype=torch.float64, device=self.X.device)
            self.X.copy_(x0.expand(self.shape))
        else:
            torch.mul(X0.expand(self.shape), _free_mask(topo), out=self.X)
        _mass_apply(self.mass, self.B * p, p, self.X, self.R)
        self.lam.fill_(math.inf)
        self.n_run = 0

    def advance(self, factor: FrameFactor, n: int) -> None:
        """n times (re-solve of the B * p rows on `factor`, mass apply, Ritz step) on the current stream: no readback, no allocation."""
        topo, p, dev = self.topo, self.p, self.X.device
        lib = _cabi.load()
        for _ in range(n):
            _resolve_launch(factor, p, self.R, p * topo.Nn * 3, self.out)
            _mass_apply(self.mass, self.B * p, p, self.X, self.MX)
            with torch.cuda.device(dev):
                rc = lib.ops_frame_modes_ritz_f64(self.B, p, topo.Nn, self.X.data_ptr(), self.MX.data_ptr(), self.R.data_ptr(), self.Q.data_ptr(),
                                                  self.lam.data_ptr(), self.change.data_ptr(), self.out.status.data_ptr(), self.status.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream)
            _cabi.check(rc, "ops_frame_modes_ritz_f64")
            self.n_run += 1

    def result(self, m: int) -> FrameModes:
        """The m lowest pairs as new tensors, the sign of a shape making its component of largest magnitude positive."""
        shapes = self.Q[:, :m].clone(memory_format=torch.contiguous_format)
        flat = shapes.view(self.B, m, -1)
        lead = flat.gather(2, flat.abs().argmax(dim=2, keepdim=True))          # (the first of equal maxima)
        flat.mul_(torch.where(lead < 0.0, -1.0, 1.0))
        eig = self.lam[:, :m].clone()
        return FrameModes(eig, torch.sqrt(eig) / (2.0 * math.pi), shapes, self.change[:, :m].clone(), self.n_run, self.status.clone())


def frame_modes(factor: FrameFactor, mass: FrameMass, n_modes: int = 1, n_vectors: Optional[int] = None, iters: Optional[int] = None,
                tol: float = 1e-10, max_iters: int = 64, poll_every: int = 4, X0: Optional[torch.Tensor] = None) -> FrameModes:
    """The `n_modes` lowest eigenpairs of K(I_b) phi = lambda M phi for the B frames of a kept factorisation, by subspace iteration on
    `n_vectors` vectors (m <= p <= min(8, n_eq); default min(8, n_eq, max(2 m, m + 4))).  Per iteration three launches on the current
    stream: the re-solve of all B * p rows, the mass apply, the Ritz step (one wavefront per frame).  With `iters` exactly that many
    iterations run and nothing is read back; otherwise the loop ends when `change <= tol` for the m requested modes of every frame
    with status 0, looked at every `poll_every` iterations, or after `max_iters`.  `change` is the relative difference of a Ritz value
    between two iterations: it is NOT an error bound -- where modes are close together a Ritz value can stand still long before it has
    converged.  The start is `default_start` unless `X0` (float64 [p,Nn,3] or [B,p,Nn,3]; its values on constrained DOFs are zeroed)
    is given.  The modes are M-normalised and their sign makes the component of largest magnitude positive (the lowest node-major
    index on a tie).  A frame whose factorisation failed is NaN with status 1; a frame whose X^T M X is not positive definite is NaN
    with status 2; neither touches another frame.  Status 2 has two causes: p exceeds the number of DOFs that carry mass (possible
    with lumped mass), or the start vectors are numerically dependent after one solve -- which the DEFAULT start is when p equals
    the number of equations (the 1 x 1 frame, six equations, with n_modes=2 and the default n_vectors = 6: cond(X^T M X) is 1e17
    there); pass a smaller `n_vectors` or an `X0` of your own (unit vectors of the free DOFs serve) on such a frame.  The
    iteration's buffers are kept on the factor by shape; the results are new tensors."""
    topo, I = factor.topo, factor.I
    B, dev = I.shape[0], I.device
    if not isinstance(mass, FrameMass) or mass.topo is not topo:
        raise ValueError("mass must be a FrameMass of the factor's topology")
    m = int(n_modes)
    p = default_vectors(topo, m) if n_vectors is None else int(n_vectors)
    if m < 1 or not m <= p <= min(MAX_VECTORS, topo.n_eq):
        raise ValueError(f"1 <= n_modes <= n_vectors <= min({MAX_VECTORS}, n_eq = {topo.n_eq}) needed, got n_modes = {m}, n_vectors = {p}")
    if mass.batch is not None and mass.batch != B:
        raise ValueError(f"nodal_mass is per frame for {mass.batch} frames, the factor holds {B}")
    if iters is not None and int(iters) < 1:
        raise ValueError("iters must be >= 1")
    if iters is None and (int(max_iters) < 1 or int(poll_every) < 1 or not tol > 0.0):
        raise ValueError("max_iters >= 1, poll_every >= 1 and tol > 0 needed")
    if X0 is not None and not (torch.is_tensor(X0) and X0.dtype == torch.float64 and tuple(X0.shape) in ((p, topo.Nn, 3), (B, p, topo.Nn, 3))):
        raise ValueError(f"X0 must be float64 [{p}, {topo.Nn}, 3] or [{B}, {p}, {topo.Nn}, 3]")
    if not I.is_cuda or (X0 is not None and not X0.is_cuda):
        raise RuntimeError("frame_modes needs GPU tensors: openpystruct_amd has no CPU fallback")
    if mass.d_mass.device != dev or (X0 is not None and X0.device != dev):
        raise ValueError(f"the mass tables and X0 must be on {dev}, where the factor is")
    lib = _cabi.load()
    f64 = dict(dtype=torch.float64, device=dev)
    if B == 0:
        e = torch.empty((0, m), **f64)
        return FrameModes(e, e.clone(), torch.empty((0, m, topo.Nn, 3), **f64), e.clone(), 0, torch.empty((0,), dtype=torch.int32, device=dev))
    it = _ModeIteration(topo, mass, B, p, factor._buffer)
    it.start(X0)
    for _ in range(int(iters) if iters is not None else int(max_iters)):
        it.advance(factor, 1)
        if iters is None and it.n_run % int(poll_every) == 0:
            if bool(((it.status != 0) | (it.change[:, :m] <= tol).all(dim=1)).all()):
                break
    return it.result(m)


def frame_solve_modes(topo: FrameTopology, I: torch.Tensor, mass: FrameMass, **kwargs) -> FrameModes:
    """`frame_modes(frame_factor(topo, I), mass, ...)`: one factorisation per frame, then the iteration.  The limits are those of
    `frame_factor` (half bandwidth <= 55)."""
    if not isinstance(mass, FrameMass) or mass.topo is not topo:
        raise ValueError("mass must be a FrameMass of this topology")
    return frame_modes(frame_factor(topo, I), mass, **kwargs)


def _modes_grad(topo: FrameTopology, shapes: torch.Tensor, status: torch.Tensor, g_eigenvalues: torch.Tensor) -> torch.Tensor:
    """ops_frame_modes_grad_f64 on the current stream: gI [B,Ne] from M-normalised shapes [B,m,Nn,3] and g_eigenvalues [B,m]."""
    if not (torch.is_tensor(shapes) and shapes.dtype == torch.float64 and shapes.dim() == 4 and tuple(shapes.shape[2:]) == (topo.Nn, 3)
            and 1 <= shapes.shape[1] <= MAX_VECTORS):
        raise ValueError(f"shapes must be float64 [B, m, {topo.Nn}, 3] with 1 <= m <= {MAX_VECTORS}")
    B, m = shapes.shape[:2]
    g = _checked("g_eigenvalues", g_eigenvalues, torch.float64, (B, m))
    status = _checked("status", status, torch.int32, (B,))
    if not shapes.is_cuda or not g.is_cuda or not status.is_cuda:
        raise RuntimeError("frame_modes_vjp needs GPU tensors: openpystruct_amd has no CPU fallback")
    dev = shapes.device
    if g.device != dev or status.device != dev:
        raise ValueError(f"g_eigenvalues and status must be on {dev}, where the shapes are")
    shapes = shapes.contiguous()
    adj = _adjoint_tables(topo)
    gI = torch.empty((B, topo.Ne), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _cabi.load().ops_frame_modes_grad_f64(B, m, m, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(), adj.conn.data_ptr(),
                                                   shapes.data_ptr(), g.data_ptr(), status.data_ptr(), gI.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_frame_modes_grad_f64")
    return gI


def frame_modes_vjp(factor: FrameFactor, modes: FrameModes, g_eigenvalues: torch.Tensor) -> torch.Tensor:
    """gI [B,Ne] = sum_j g_eigenvalues[b,j] dlambda_j/dI_e with dlambda_j/dI_e = phi_j,e . (K_b,e phi_j,e): M does not depend on I, so a
    frequency costs one streaming launch to differentiate and no adjoint solve.  Defined only where the eigenvalue is simple; a
    frame with a non-zero status gets a NaN row."""
    return _modes_grad(factor.topo, modes.shapes, modes.status, g_eigenvalues)


def differentiable_frame_frequencies(topo: FrameTopology, I: torch.Tensor, mass: FrameMass, n_modes: int = 1,
                                     n_vectors: Optional[int] = None, iters: Optional[int] = None, tol: float = 1e-10,
                                     max_iters: int = 64, poll_every: int = 4, X0: Optional[torch.Tensor] = None):
    """(eigenvalues [B,m], frequencies [B,m] in Hz) of `frame_solve_modes` through the registered operator
    `openpystruct_amd::frame_eigenvalues` (torch_op.py): gradients reach I.  The gradient of a single eigenvalue is defined only
    where that eigenvalue is simple: at a repeated eigenvalue only symmetric functions of the cluster (their sum, for one) are
    differentiable, and what comes back there depends on the basis the iteration happened to return.  The mode shapes carry no
    gradient.  The graph keeps `topo` and `mass` alive until it is freed."""
    from . import torch_op
    return torch_op.frame_frequencies_autograd(topo, I, mass, n_modes, n_vectors, iters, tol, max_iters, poll_every, X0)
