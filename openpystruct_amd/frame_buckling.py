"""Linear buckling load factors of batched 2-D frames on the kept factorisation.

The eigenproblem is K(I) phi = lambda S(N) phi on the free DOFs, K the matrix `frame_factor` factorises and S = -K_g(N) the negated
geometric stiffness of the member axial forces N_e (tension positive) of a reference static solution of the same frames.  The
critical load factors are the positive lambda, ascending: the factor by which the reference loads can grow before the frame
buckles.  S is indefinite (members in tension) and can be rank deficient, so the roles of the two matrices are swapped against
`frame_modes`: an inverse iteration on K^-1 S with a Ritz step whose Cholesky factor is that of X^T K X.  Per iteration the
re-solve of `frame_resolve` with the right-hand sides S Q, the geometric-stiffness apply and the Ritz step of csrc/frame_loads.hip
(arithmetic: csrc/frame_buckling.hpp) -- three launches, no factorisation, no CPU path.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import _cabi
from .frame_modes import MAX_VECTORS, _free_mask, default_start, default_vectors
from .frames import (FrameCaseSolution, FrameFactor, FrameSolution, FrameTopology, _adjoint_tables, _checked, _resolve_launch, frame_factor,
                     frame_solve_cases_vjp)

KINDS = ("consistent", "pdelta")


class FrameBuckling(NamedTuple):
    load_factors: torch.Tensor   # [B, m]        lambda = 1 / mu where mu > 0, else +inf, ascending
    mu: torch.Tensor             # [B, m]        phi^T S phi, descending
    shapes: torch.Tensor         # [B, m, Nn, 3] phi^T K phi = 1; the component of largest magnitude is positive
    change: torch.Tensor         # [B, m]        |mu - mu of the iteration before| / |mu|
    iterations: int
    status: torch.Tensor         # [B] int32     0; 1: the factorisation, the reference solve or a re-solve failed; 2: X^T K X not positive definite
    reference: FrameSolution     # the static solution whose axial forces S was built from
    kind: str                    # "consistent" or "pdelta": the geometric matrix


def _geom_apply(topo: FrameTopology, forces: torch.Tensor, consistent: int, rows: int, rows_per_frame: int, x: torch.Tensor,
                y: torch.Tensor) -> None:
    """ops_frame_geom_apply_f64 on the current stream: y[r] = S x[r] for `rows` rows [Nn,3]."""
    adj = _adjoint_tables(topo)
    dev = x.device
    with torch.cuda.device(dev):
        rc = _cabi.load().ops_frame_geom_apply_f64(
            rows, rows_per_frame, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), adj.conn.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr(),
            forces.data_ptr(), consistent, x.data_ptr(), y.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_frame_geom_apply_f64")


def _checked_reference(topo: FrameTopology, reference, B: int) -> FrameSolution:
    if not isinstance(reference, FrameSolution):
        raise ValueError("reference must be a FrameSolution of the factor's frames (one case of frame_resolve serves), or None")
    return FrameSolution(_checked("reference.disp", reference.disp, torch.float64, (B, topo.Nn, 3)),
                         _checked("reference.forces", reference.forces, torch.float64, (B, topo.Ne, 6)), reference.V, reference.M,
                         _checked("reference.status", reference.status, torch.int32, (B,)))


def frame_buckling(factor: FrameFactor, n_modes: int = 1, reference: Optional[FrameSolution] = None, kind: str = "consistent",
                   n_vectors: Optional[int] = None, iters: Optional[int] = None, tol: float = 1e-10, max_iters: int = 64,
                   poll_every: int = 4, X0: Optional[torch.Tensor] = None) -> FrameBuckling:
    """The `n_modes` lowest critical load factors of the B frames of a kept factorisation: K(I_b) phi = lambda S phi, S the negated
    geometric stiffness of the axial forces of `reference` -- None: the factor's keeping solution, under the topology's own loads;
    otherwise a `FrameSolution` of the same B frames and the same I (one case of `frame_resolve`, say).  `kind`: "consistent" (the
    cubic-shape matrix on (v1, th1, v2, th2), error of order h^4 in the element length) or "pdelta" (N / L [[1, -1], [-1, 1]] on the
    transverse translations, the linearised P-Delta matrix, order h^2).  The iteration runs on `n_vectors` vectors (m <= p <=
    min(8, n_eq); default min(8, n_eq, max(2 m, m + 4))); per iteration three launches on the current stream: the re-solve of all
    B * p rows, the geometric apply, the Ritz step (one wavefront per frame).  `iters`, `tol`, `max_iters`, `poll_every` and `X0` are
    those of `frame_modes`; `change` is the relative difference of mu = 1 / lambda between two iterations and NOT an error bound.
    The iteration converges to the eigenvalues of K^-1 S of largest MAGNITUDE, so its rate is governed by |mu|, not mu: a load state
    with strongly tensioned members (large negative mu) slows the positive modes, which are the ones returned first, and more
    vectors are the remedy.  A mode whose mu is not positive has load factor +inf: no buckling in that mode under this load
    direction.  The shapes are K-normalised (phi^T K phi = 1, so phi^T S phi = mu) with the sign rule of `frame_modes`.  A frame
    whose factorisation or reference solve failed is NaN with status 1; a frame whose X^T K X is not positive definite (a Cholesky pivot at or
    below 2^-40 of its diagonal entry) is NaN with status 2: p exceeds the rank of S ("pdelta" carries nothing on rotations: the 1 x 1 frame has an S of rank 3, use p <= 3 there) or
    the start vectors are dependent; neither touches another frame.  The iteration's buffers are kept on the factor by shape; the
    results are new tensors."""
    topo, I = factor.topo, factor.I
    B, dev = I.shape[0], I.device
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}")
    m = int(n_modes)
    p = default_vectors(topo, m) if n_vectors is None else int(n_vectors)
    if m < 1 or not m <= p <= min(MAX_VECTORS, topo.n_eq):
        raise ValueError(f"1 <= n_modes <= n_vectors <= min({MAX_VECTORS}, n_eq = {topo.n_eq}) needed, got n_modes = {m}, n_vectors = {p}")
    if iters is not None and int(iters) < 1:
        raise ValueError("iters must be >= 1")
    if iters is None and (int(max_iters) < 1 or int(poll_every) < 1 or not tol > 0.0):
        raise ValueError("max_iters >= 1, poll_every >= 1 and tol > 0 needed")
    if X0 is not None and not (torch.is_tensor(X0) and X0.dtype == torch.float64 and tuple(X0.shape) in ((p, topo.Nn, 3), (B, p, topo.Nn, 3))):
        raise ValueError(f"X0 must be float64 [{p}, {topo.Nn}, 3] or [{B}, {p}, {topo.Nn}, 3]")
    own = reference is None
    ref = factor.solution if own else _checked_reference(topo, reference, B)
    if not I.is_cuda or (X0 is not None and not X0.is_cuda) or not ref.forces.is_cuda:
        raise RuntimeError("frame_buckling needs GPU tensors: openpystruct_amd has no CPU fallback")
    if ref.forces.device != dev or ref.status.device != dev or (X0 is not None and X0.device != dev):
        raise ValueError(f"the reference and X0 must be on {dev}, where the factor is")
    lib = _cabi.load()
    f64 = dict(dtype=torch.float64, device=dev)
    if B == 0:
        e = torch.empty((0, m), **f64)
        return FrameBuckling(e, e.clone(), torch.empty((0, m, topo.Nn, 3), **f64), e.clone(), 0, torch.empty((0,), dtype=torch.int32, device=dev), ref, kind)
    consistent = int(kind == "consistent")
    shape = (B, p, topo.Nn, 3)
    out = FrameCaseSolution(factor._buffer("buckling_X", shape), factor._buffer("buckling_forces", (B, p, topo.Ne, 6)),
                            factor._buffer("buckling_V", (B, p, topo.Ne)), factor._buffer("buckling_M", (B, p, topo.Ne)),
                            factor._buffer("buckling_row_status", (B, p), torch.int32))
    X, SX, R, Q = out.disp, factor._buffer("buckling_SX", shape), factor._buffer("buckling_R", shape), factor._buffer("buckling_Q", shape)
    mu, lam, change = (factor._buffer(f"buckling_{k}", (B, p)) for k in ("mu", "lambda", "change"))
    status = factor._buffer("buckling_status", (B,), torch.int32)
    if X0 is None:
        x0 = topo.__dict__.setdefault("_modes_x0", {}).get(p)
        if x0 is None:
            x0 = topo.__dict__["_modes_x0"][p] = torch.as_tensor(default_start(topo, p), **f64)
        X.copy_(x0.expand(shape))
    else:
        torch.mul(X0.expand(shape), _free_mask(topo), out=X)
    _geom_apply(topo, ref.forces, consistent, B * p, p, X, R)
    mu.fill_(math.inf)
    n_run = 0
    for it in range(int(iters) if iters is not None else int(max_iters)):
        _resolve_launch(factor, p, R, p * topo.Nn * 3, out)
        _geom_apply(topo, ref.forces, consistent, B * p, p, X, SX)
        with torch.cuda.device(dev):
            rc = lib.ops_frame_buckling_ritz_f64(B, p, topo.Nn, X.data_ptr(), SX.data_ptr(), R.data_ptr(), Q.data_ptr(), mu.data_ptr(),
                                                 lam.data_ptr(), change.data_ptr(), out.status.data_ptr(), status.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(rc, "ops_frame_buckling_ritz_f64")
        n_run = it + 1
        if iters is None and n_run % int(poll_every) == 0:
            if bool(((status != 0) | (change[:, :m] <= tol).all(dim=1)).all()):
                break
    shapes = Q[:, :m].clone(memory_format=torch.contiguous_format)
    flat = shapes.view(B, m, -1)
    lead = flat.gather(2, flat.abs().argmax(dim=2, keepdim=True))          # (the first of equal maxima)
    flat.mul_(torch.where(lead < 0.0, -1.0, 1.0))
    st = status.clone()
    if not own:          # a reference whose own solve failed holds NaN forces: S is NaN and the Ritz step reports 2
        st = torch.where(ref.status != 0, torch.ones_like(st), st)
    return FrameBuckling(lam[:, :m].clone(), mu[:, :m].clone(), shapes, change[:, :m].clone(), n_run, st, ref, kind)


def frame_solve_buckling(topo: FrameTopology, I: torch.Tensor, **kwargs) -> FrameBuckling:
    """`frame_buckling(frame_factor(topo, I), ...)`: one factorisation per frame, then the iteration.  The limits are those of
    `frame_factor` (half bandwidth <= 55)."""
    return frame_buckling(frame_factor(topo, I), **kwargs)


def _buckling_grad(topo: FrameTopology, kind: str, shapes: torch.Tensor, load_factors: torch.Tensor, status: torch.Tensor,
                   g_load_factors: torch.Tensor):
    """ops_frame_buckling_grad_f64 on the current stream: (gI_direct [B,Ne], g_forces [B,Ne,6]) from K-normalised shapes [B,m,Nn,3]."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}")
    if not (torch.is_tensor(shapes) and shapes.dtype == torch.float64 and shapes.dim() == 4 and tuple(shapes.shape[2:]) == (topo.Nn, 3)
            and 1 <= shapes.shape[1] <= MAX_VECTORS):
        raise ValueError(f"shapes must be float64 [B, m, {topo.Nn}, 3] with 1 <= m <= {MAX_VECTORS}")
    B, m = shapes.shape[:2]
    lam = _checked("load_factors", load_factors, torch.float64, (B, m))
    g = _checked("g_load_factors", g_load_factors, torch.float64, (B, m))
    status = _checked("status", status, torch.int32, (B,))
    if not shapes.is_cuda or not lam.is_cuda or not g.is_cuda or not status.is_cuda:
        raise RuntimeError("frame_buckling_vjp needs GPU tensors: openpystruct_amd has no CPU fallback")
    dev = shapes.device
    if lam.device != dev or g.device != dev or status.device != dev:
        raise ValueError(f"load_factors, g_load_factors and status must be on {dev}, where the shapes are")
    shapes = shapes.contiguous()
    adj = _adjoint_tables(topo)
    direct = torch.empty((B, topo.Ne), dtype=torch.float64, device=dev)
    g_forces = torch.empty((B, topo.Ne, 6), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _cabi.load().ops_frame_buckling_grad_f64(B, m, m, topo.Nn, topo.Ne, topo.d_geo.data_ptr(), topo.d_E.data_ptr(),
                                                      adj.conn.data_ptr(), int(kind == "consistent"), shapes.data_ptr(), lam.data_ptr(),
                                                      g.data_ptr(), status.data_ptr(), direct.data_ptr(), g_forces.data_ptr(),
                                                      torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(rc, "ops_frame_buckling_grad_f64")
    return direct, g_forces


def frame_buckling_vjp(factor: FrameFactor, result: FrameBuckling, g_load_factors: torch.Tensor):
    """(gI [B,Ne], g_loads [B,Nn,3], g_element_loads [B,Ne,2]) = sum_j g_load_factors[b,j] dlambda_j / d(I, loads, element loads of the
    reference solve), with dlambda_j/dI_e = lambda_j phi_j,e . (K_b,e phi_j,e) + lambda_j^2 sum_e' w_j,e' dN_e'/dI_e, w = phi . (k_g,unit
    phi): in a statically indeterminate frame the axial forces depend on I, so unlike a frequency a load factor does need the
    adjoint.  One streaming launch (the first term and the cotangent of the reference's end forces), then `frame_solve_cases_vjp`
    on the reference viewed as one case: one adjoint re-solve on the kept factor and no factorisation.  A mode with load factor +inf contributes nothing; a frame with a non-zero status gets NaN rows.
    The gradient of a single load factor is defined only where that eigenvalue is simple: at a repeated eigenvalue only symmetric
    functions of the cluster are differentiable, and what comes back there depends on the basis the iteration happened to return."""
    topo = factor.topo
    direct, g_forces = _buckling_grad(topo, result.kind, result.shapes, result.load_factors, result.status, g_load_factors)
    ref = result.reference
    sol = FrameCaseSolution(ref.disp.unsqueeze(1), ref.forces.unsqueeze(1), None, None, ref.status.unsqueeze(1))
    gI, g_loads, g_w = frame_solve_cases_vjp(factor, sol, g_forces=g_forces.unsqueeze(1))
    return direct + gI, g_loads[:, 0], g_w[:, 0]


def differentiable_frame_buckling(topo: FrameTopology, I: torch.Tensor, n_modes: int = 1, kind: str = "consistent",
                                  n_vectors: Optional[int] = None, iters: Optional[int] = None, tol: float = 1e-10,
                                  max_iters: int = 64, poll_every: int = 4, X0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The load factors [B,m] of `frame_solve_buckling` under the topology's own loads through the registered operator
    `openpystruct_amd::frame_buckling_factors` (torch_op.py): gradients reach I.  The gradient of a single load factor is defined only
    where that eigenvalue is simple: at a repeated eigenvalue only symmetric functions of the cluster (their sum, for one) are
    differentiable, and what comes back there depends on the basis the iteration happened to return.  A load factor of +inf has a
    zero gradient.  The mode shapes carry no gradient.  The graph keeps `topo` alive until it is freed."""
    from . import torch_op
    return torch_op.frame_buckling_autograd(topo, I, n_modes, kind, n_vectors, iters, tol, max_iters, poll_every, X0)
