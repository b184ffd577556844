"""Natural frequencies and mode shapes on the host (no GPU): (a) the dense reference (tests/frame_modes_ref.py)
against the closed form of a cantilever and its gradient formula against central differences; (b) the arithmetic of
csrc/frame_modes.hpp -- the text the HIP kernels of csrc/frame_loads.hip compile -- built with g++ and the address +
undefined-behaviour sanitizers into a stand-alone program: node mass rows, the whole Ritz step (the 64 lanes one after the other,
their partial sums added by the kernel's butterfly) and the gradient rows against the reference; (c) the binding, the refusals
of the three C entries (decided before any HIP call: no device is needed), the argument checks of the Python entries and what the
command shim records; (d) the conditions the GPU tests (tests/test_gpu_frame_modes.py) rely on, on the reference alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import frame_dense as fd  # noqa: E402
from tests import frame_modes_ref as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpystruct_amd", "csrc")
HEADER = os.path.join(CSRC, "frame_modes.hpp")
KEYS = list(fr.CASES)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the reference itself
# ---------------------------------------------------------------------------------------------------------------------
def _cantilever(n_el, kind):
    """A fixed-base vertical cantilever, 8 m, EI = 1e8, 157 kg/m: the first two bending eigenvalues (EA = 2e12 keeps the first
    axial mode far above them)."""
    H, EI, mbar = 8.0, 1e8, 157.0
    coords = np.array([(0.0, H * i / n_el) for i in range(n_el + 1)])
    conn = np.array([(i, i + 1) for i in range(n_el)])
    fix3 = np.zeros((n_el + 1, 3), dtype=bool); fix3[0] = True
    z = np.zeros(n_el)
    case = fd.FrameCase(coords, conn, fix3, np.full(n_el, 1.0), np.full(n_el, 2e12), z, z, np.zeros((n_el + 1, 3)))
    I = np.full(n_el, EI / 2e12)
    lam, phi = fr.dense_modes(case, I, fr.dense_M(case, mbar, kind), 6)
    bending = [j for j in range(6) if np.abs(phi[j].reshape(-1, 3)[:, 0]).max() > 10 * np.abs(phi[j].reshape(-1, 3)[:, 1]).max()][:2]
    exact = np.array([1.8751040687, 4.6940911330]) ** 4 * EI / (mbar * H ** 4)
    return (lam[bending] - exact) / exact


def test_cantilever_closed_form_and_order_of_convergence():
    """Measured: consistent, first mode 4.2e-6 at 8 elements and 2.6e-7 at 16 (order h^4); lumped -1.4e-2 and -3.6e-3 (order h^2)."""
    c8, c16, l8, l16 = _cantilever(8, "consistent"), _cantilever(16, "consistent"), _cantilever(8, "lumped"), _cantilever(16, "lumped")
    print(f"consistent {c8} {c16} lumped {l8} {l16}")
    assert 0.0 < c16[0] < 1e-6 and 0.0 < c16[1] < 1e-4
    assert 12.0 <= c8[0] / c16[0] <= 20.0
    assert l8[0] < 0.0 and 3.0 <= l8[0] / l16[0] <= 5.0


@pytest.mark.parametrize("key", ["1x1-c", "3x6-l", "10x4n-c", "general-c", "hub-c"])
def test_gradient_formula_matches_central_differences(key):
    """dlambda_j/dI_e = phi_j,e^T K_b,e phi_j,e against (lambda(I + h e_e) - lambda(I - h e_e)) / 2h, h = 1e-4 I_e: the truncation error
    of the difference is O(h^2) relative, its rounding error 1e-16 / 1e-4 relative to lambda / I_e."""
    case, I, mbar, nodal, kind, _ = fr.inputs(key)
    M = fr.dense_M(case, mbar, kind, fr.nodal_of(nodal, 0))
    lam, phi = fr.dense_modes(case, I[0], M, 2)
    g = fr.dlambda_dI(case, phi)
    for e in range(0, I.shape[1], max(1, I.shape[1] // 5)):
        h = 1e-4 * I[0, e]
        up, dn = I[0].copy(), I[0].copy()
        up[e] += h; dn[e] -= h
        num = (fr.dense_modes(case, up, M, 2)[0] - fr.dense_modes(case, dn, M, 2)[0]) / (2 * h)
        assert np.all(np.abs(num - g[:, e]) <= 1e-6 * np.abs(g[:, e]) + 1e-9 * lam / I[0, e]), (e, num, g[:, e])


# ---------------------------------------------------------------------------------------------------------------------
# (b) csrc/frame_modes.hpp with g++
# ---------------------------------------------------------------------------------------------------------------------
_PROGRAM = r"""
#include "frame_modes.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace opsamd;
template <class T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short file\n"); std::exit(2); }
  return v;
}
// one frame's Ritz step as the kernel runs it: the lanes' partial sums, the butterfly over the 64 lanes (lane 0's result), the
// small part, the lanes' entries of Q and R.  out: q [P,n], r [P,n], lam [P], change [P], status, sweeps
template <int P>
static void ritz(long n, const double* x, const double* mx, std::vector<double> r, const double* prev, std::vector<double>& out) {
  constexpr int NA = FmRitz<P>::NACC;
  std::vector<double> part((size_t)FM_LANES * NA), next(part.size());
  for (int lane = 0; lane < FM_LANES; ++lane) fm_ritz_partials<P>(n, x, mx, r.data(), lane, part.data() + (size_t)lane * NA);
  for (int off = 32; off >= 1; off >>= 1) {
    for (int lane = 0; lane < FM_LANES; ++lane)
      for (int k = 0; k < NA; ++k) next[(size_t)lane * NA + k] = part[(size_t)lane * NA + k] + part[(size_t)(lane ^ off) * NA + k];
    part.swap(next);
  }
  for (int lane = 1; lane < FM_LANES; ++lane)
    for (int k = 0; k < NA; ++k)
      if (part[(size_t)lane * NA + k] != part[k] && part[k] == part[k]) { std::fprintf(stderr, "lanes differ\n"); std::exit(3); }
  double Z[P * P], lam[P], change[P];
  int sweeps = -1;
  const int st = fm_ritz_small<P>(part.data(), prev, Z, lam, change, &sweeps);
  std::vector<double> q((size_t)P * n, __builtin_nan(""));
  if (st == 0)
    for (int lane = 0; lane < FM_LANES; ++lane) fm_ritz_update<P>(n, x, mx, Z, lane, q.data(), r.data());
  out.insert(out.end(), q.begin(), q.end());
  out.insert(out.end(), r.begin(), r.end());
  for (int j = 0; j < P; ++j) out.push_back(st == 0 ? lam[j] : __builtin_nan(""));
  for (int j = 0; j < P; ++j) out.push_back(st == 0 ? change[j] : __builtin_nan(""));
  out.push_back(st);
  out.push_back(sweeps);
}
// <in> <out>.  in: int32 mode (0: mass rows, 1: Ritz, 2: gradient rows), R | B, rows_per_frame | p, Nn, Ne, consistent | m, nodal (0: none,
// 1: shared, 2: per frame); geo, E; conn, ptr, idx; mode 0: elem_mass, nodal, x; mode 1: X, MX, R, lambda_prev; mode 2: phi, g, status
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = rd<int32_t>(f, 7);
  const int mode = h[0], R = h[1], rpf = h[2], Nn = h[3], Ne = h[4], flag = h[5], nodal = h[6];
  const auto geo = rd<double>(f, 3 * (size_t)Ne), E = rd<double>(f, Ne);
  const auto conn = rd<int32_t>(f, 2 * (size_t)Ne), ptr = rd<int32_t>(f, Nn + 1), idx = rd<int32_t>(f, 2 * (size_t)Ne);
  std::vector<double> out;
  if (mode == 0) {
    const int frames = (R + rpf - 1) / rpf;
    const auto mass = rd<double>(f, Ne), nm = rd<double>(f, nodal == 0 ? 0 : (size_t)(nodal == 1 ? 1 : frames) * Nn * 3);
    const auto x = rd<double>(f, (size_t)R * Nn * 3);
    for (long r = 0; r < R; ++r)
      for (int n = 0; n < Nn; ++n) {
        double y[3];
        fm_node_mass(Nn, geo.data(), conn.data(), ptr.data(), idx.data(), mass.data(), flag, nodal ? nm.data() : nullptr,
                     nodal == 2 ? 3L * Nn : 0L, x.data(), r, r / rpf, n, y);
        out.insert(out.end(), y, y + 3);
      }
  } else if (mode == 1) {
    const int B = R, p = rpf;
    const long n = 3L * Nn;
    const auto X = rd<double>(f, (size_t)B * p * n), MX = rd<double>(f, (size_t)B * p * n), Rr = rd<double>(f, (size_t)B * p * n);
    const auto prev = rd<double>(f, (size_t)B * p);
    for (long b = 0; b < B; ++b) {
      const double *x = X.data() + b * p * n, *mx = MX.data() + b * p * n, *pv = prev.data() + b * p;
      const std::vector<double> r(Rr.begin() + b * p * n, Rr.begin() + (b + 1) * p * n);
      switch (p) {
        case 1: ritz<1>(n, x, mx, r, pv, out); break;
        case 2: ritz<2>(n, x, mx, r, pv, out); break;
        case 3: ritz<3>(n, x, mx, r, pv, out); break;
        case 4: ritz<4>(n, x, mx, r, pv, out); break;
        case 5: ritz<5>(n, x, mx, r, pv, out); break;
        case 6: ritz<6>(n, x, mx, r, pv, out); break;
        case 7: ritz<7>(n, x, mx, r, pv, out); break;
        case 8: ritz<8>(n, x, mx, r, pv, out); break;
        default: return 2;
      }
    }
  } else {
    const int B = R, p = rpf, m = flag;
    const auto phi = rd<double>(f, (size_t)B * p * Nn * 3), g = rd<double>(f, (size_t)B * m);
    for (long b = 0; b < B; ++b)
      for (int e = 0; e < Ne; ++e) out.push_back(fm_elem_grad(m, p, Nn, geo.data(), E.data(), conn.data(), phi.data(), g.data(), b, e));
  }
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) return 2;
  std::fclose(o);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found: the host program cannot be built")
    assert os.path.exists(HEADER), "csrc/frame_modes.hpp is missing"
    d = tmp_path_factory.mktemp("frame_modes")
    src, exe = d / "frame_modes_host.cpp", d / "frame_modes_host"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _run(program, tmp_path, topo, head, arrays):
    from openpystruct_amd import frames
    adj = frames._adjoint_tables(topo)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array(head, dtype=np.int32).tofile(f)
        topo.d_geo.numpy().astype(np.float64).tofile(f)
        topo.d_E.numpy().astype(np.float64).tofile(f)
        for t in (adj.conn, adj.ptr, adj.idx):
            t.numpy().astype(np.int32).tofile(f)
        for a in arrays:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    subprocess.check_call([program, str(fin), str(fout)])
    return np.fromfile(fout, dtype=np.float64)


def _topo(key):
    return fr.topology(fr.CASES[key][0], "cpu")


def host_mass_rows(program, tmp_path, key, x, rows_per_frame):
    """y [R,Nn,3] = M x from the g++ build, for the inputs of a shared case."""
    topo = _topo(key)
    _, _, mbar, nodal, kind, _ = fr.inputs(key)
    R = x.shape[0]
    nod = 0 if nodal is None else nodal.ndim - 1
    arrays = [mbar] + ([] if nodal is None else [nodal]) + [x]
    return _run(program, tmp_path, topo, [0, R, rows_per_frame, topo.Nn, topo.Ne, kind == "consistent", nod], arrays).reshape(R, topo.Nn, 3)


def host_grad_rows(program, tmp_path, key, phi, g):
    topo = _topo(key)
    B, m = g.shape
    return _run(program, tmp_path, topo, [2, B, phi.shape[1], topo.Nn, topo.Ne, m, 0], [phi, g]).reshape(B, topo.Ne)


def _mass_ratio(program, tmp_path, key):
    """Largest elementwise |got - ref| / (2^-52 |M| |x|) of the g++ build against dense M @ x on a shared case's inputs."""
    case, I, mbar, nodal, kind, p = fr.inputs(key)
    B = I.shape[0]
    x = fr.mass_apply_x(key)
    y = host_mass_rows(program, tmp_path, key, x.reshape(B * 3, -1, 3), 3).reshape(B, 3, -1)
    worst = 0.0
    for b in range(B):
        M = fr.dense_M(case, mbar, kind, fr.nodal_of(nodal, b))
        ref, scale = x[b] @ M.T, np.abs(x[b]) @ np.abs(M).T
        worst = max(worst, float((np.abs(y[b] - ref) / (fr.EPS * np.maximum(scale, 1e-300)))[scale > 0].max()))
        assert np.all(y[b][scale == 0] == 0.0)
    return worst


def _grad_ratio(program, tmp_path, key):
    """Largest elementwise |got - ref| / (2^-52 sum_j |g_j| |phi|^T |K_b| |phi|) of the g++ build, fed the reference's phi."""
    case, I, _, _, _, _ = fr.inputs(key)
    ref = fr.reference(key)
    phi = np.stack([r["phi"] for r in ref])                                  # [B,2,3Nn]
    g = fr.grad_cotangent(key)
    got = host_grad_rows(program, tmp_path, key, phi, g)
    worst = 0.0
    for b in range(I.shape[0]):
        worst = max(worst, float((np.abs(got[b] - g[b] @ ref[b]["dl"]) / (fr.EPS * fr.grad_scale(case, phi[b], g[b]))).max()))
    return worst


@pytest.mark.parametrize("key", KEYS)
def test_host_mass_rows_match_the_dense_mass_matrix(program, tmp_path, key):
    """Elementwise against dense M @ x, relative to 2^-52 (|M| |x|).  Measured: at most 2.6897 (10x4n-c)."""
    worst = _mass_ratio(program, tmp_path, key)
    print(f"mass apply: largest |got - ref| / (2^-52 |M||x|) = {worst:.5f}")
    assert worst <= fr.MASS_RATIO


@pytest.mark.parametrize("key", KEYS)
def test_host_gradient_rows_match_the_reference(program, tmp_path, key):
    """Fed the reference's phi: elementwise relative to 2^-52 sum_j |g_j| |phi|^T |K_b| |phi|.  Measured: at most 2.5528 (10x4n-c)."""
    worst = _grad_ratio(program, tmp_path, key)
    print(f"gradient: largest |got - ref| / (2^-52 scale) = {worst:.5f}")
    assert worst <= fr.GRAD_RATIO


def test_the_gpu_constants_are_four_times_the_largest_host_ratio(program, tmp_path):
    """C_MASS and C_GRAD of tests/frame_modes_ref.py, the constants of the elementwise GPU bounds, are 4 x the largest ratio this build
    shows over all shared cases, the ratio written down to two decimals (rounded up): pinned from below and from above."""
    mass = max(_mass_ratio(program, tmp_path, key) for key in KEYS)
    grad = max(_grad_ratio(program, tmp_path, key) for key in KEYS)
    print(f"largest ratios: mass apply {mass:.5f}, gradient {grad:.5f}")
    assert fr.MASS_RATIO - 0.01 < mass <= fr.MASS_RATIO and fr.GRAD_RATIO - 0.01 < grad <= fr.GRAD_RATIO
    assert fr.C_MASS == 4.0 * fr.MASS_RATIO and fr.C_GRAD == 4.0 * fr.GRAD_RATIO


@pytest.mark.parametrize("p", [1, 2, 5, 8])
@pytest.mark.parametrize("key", ["1x1-c", "3x6-l", "10x4n-c", "general-c", "hub-c"])
def test_host_ritz_step_matches_the_reference_iteration(program, tmp_path, key, p):
    """The whole Ritz step of iterations 1, 2 and 3 of the reference iteration on p vectors, fed the reference's X, MX and R: Ritz
    values relative 1e-9 (the bound the GPU test holds them to is 1e-8; the Ritz values of the first iteration are those of a badly
    conditioned pencil -- the start vectors are far from M-orthogonal -- so they are not held to the rounding unit), Q^T M Q = I to
    p 2^-52 cond(X^T M X), the next R = M Q, the Jacobi loop short of its cap, change = |lam - prev| / lam.
    Measured: Ritz values 1.2e-10 in the first iteration and 5e-15 after it, at most 6 sweeps."""
    case, I, mbar, nodal, kind, _ = fr.inputs(key)
    topo = _topo(key)
    p = min(p, 4 if key.startswith("1x1") else 8)      # (six equations: five start vectors give a first pencil of condition 1e13)
    B = min(I.shape[0], 3)
    n = 3 * topo.Nn
    its = []
    for b in range(B):
        M = fr.dense_M(case, mbar, kind, fr.nodal_of(nodal, b))
        its.append((M, fr.iterate(case, I[b], M, fr.default_start(case, p), 3)))
    for t in range(3):
        X, MX, R = (np.stack([its[b][1][t][k] for b in range(B)]) for k in (3, 4, 5))
        prev = np.stack([its[b][1][t - 1][0] if t else np.full(p, np.inf) for b in range(B)])
        out = _run(program, tmp_path, topo, [1, B, p, topo.Nn, topo.Ne, 0, 0], [X, MX, R, prev]).reshape(B, -1)
        for b in range(B):
            M, ref = its[b]
            q, r = out[b, :p * n].reshape(p, n), out[b, p * n:2 * p * n].reshape(p, n)
            lam, change, st, sweeps = out[b, 2 * p * n:2 * p * n + p], out[b, 2 * p * n + p:2 * p * n + 2 * p], out[b, -2], out[b, -1]
            assert st == 0 and 0 <= sweeps < 16, (t, b, st, sweeps)
            e_lam = float(np.abs(lam / ref[t][0] - 1.0).max())
            e_orth = float(np.abs(q @ M @ q.T - np.eye(p)).max())
            e_r = float(np.linalg.norm(r - q @ M.T) / np.linalg.norm(r))
            print(f"t {t + 1} frame {b}: lam {e_lam:.2e} orth {e_orth:.2e} R {e_r:.2e} sweeps {int(sweeps)}")
            assert e_lam <= 1e-9 and e_r <= 1e-12 and np.all(np.diff(lam) >= 0.0)
            cond = float(np.linalg.cond(X[b] @ M @ X[b].T))
            assert e_orth <= 1e-14 + p * fr.EPS * cond, (e_orth, cond)        # Z^T Mr Z - I from a Cholesky factor: p eps cond(Mr)
            want = np.abs(lam - prev[b]) / lam
            assert np.array_equal(change, want) and (t > 0 or np.all(np.isinf(change)))


def test_host_ritz_step_reports_a_mass_matrix_that_is_not_positive_definite(program, tmp_path):
    """Lumped mass on the 1 x 1 frame without nodal masses: four DOFs carry mass, so six vectors give status 2 and NaN; four do not."""
    topo = _topo("1x1-l")
    case, I, mbar, _, kind, _ = fr.inputs("1x1-l")
    M = fr.dense_M(case, mbar, kind)
    f = fr.free_dofs(case)
    for p, want in ((6, 2.0), (4, 0.0)):
        X0 = fr.default_start(case, p)
        R = X0 @ M.T
        X = np.zeros_like(R)
        X[:, f] = np.linalg.solve(fr.dense_K(case, I[0])[np.ix_(f, f)], R[:, f].T).T
        out = _run(program, tmp_path, topo, [1, 1, p, topo.Nn, topo.Ne, 0, 0], [X, X @ M.T, R, np.full(p, np.inf)])
        n = 3 * topo.Nn
        assert out[-2] == want
        assert bool(np.isnan(out[:p * n]).all()) == (want != 0.0) and bool(np.isnan(out[2 * p * n:2 * p * n + 2 * p]).all()) == (want != 0.0)
        if want:
            assert np.array_equal(out[p * n:2 * p * n].reshape(p, n), R)          # R stays


# ---------------------------------------------------------------------------------------------------------------------
# (c) binding, refusals, argument checks, shim
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = {"ops_frame_mass_apply_f64", "ops_frame_modes_ritz_f64", "ops_frame_modes_grad_f64"}


def test_the_entries_are_extension_exports_and_the_file_counts_hold():
    from openpystruct_amd import _cabi, build
    assert ENTRIES <= set(_cabi.EXTENSION_EXPORTS) and not ENTRIES & set(_cabi.EXPORTS)
    ext = _cabi._extensions[os.path.join(ROOT, "include", "openpystruct_amd_frame_loads.h")]
    assert ENTRIES <= set(ext.functions)
    assert len(build.SOURCES) == 26 and len(_cabi.EXTENSION_HEADER_PATHS) == 9 and len(_cabi.EXPORTS) == 70
    deps = {os.path.basename(p) for p in build._deps(os.path.join(CSRC, "frame_loads.hip"))}
    assert {"frame_modes.hpp", "frame_adjoint.hpp", "sizing_math.hpp"} <= deps


def test_c_entries_refuse_bad_arguments_without_a_device():
    """Every refusal is decided before any HIP call, so the codes come back on a machine without a GPU; the pointers are never read."""
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    x = 1 << 20                                                     # a non-NULL address that is never dereferenced
    mass = dict(R=6, rpf=2, Nn=4, Ne=3, geo=x, conn=x, ptr=x, idx=x, em=x, consistent=1, nodal=x, nbs=12, x=x, y=x, stream=None)
    ritz = dict(B=3, p=2, Nn=4, X=x, MX=x, R=x, Q=x, lam=x, change=x, rs=x, st=x, stream=None)
    grad = dict(B=3, m=2, p=2, Nn=4, Ne=3, geo=x, E=x, conn=x, phi=x, g=x, st=x, gI=x, stream=None)
    cases = [(lib.ops_frame_mass_apply_f64, mass, [{"R": -1}, {"rpf": 0}, {"Nn": 1}, {"Nn": -4}, {"Ne": 0}, {"nbs": 3}, {"nbs": -12}, {"nbs": 13}]
              + [{k: None} for k in ("geo", "conn", "ptr", "idx", "em", "x", "y")], {"R": 0, "geo": None}),
             (lib.ops_frame_modes_ritz_f64, ritz, [{"B": -1}, {"p": 0}, {"p": 9}, {"p": -2}, {"Nn": 1}]
              + [{k: None} for k in ("X", "MX", "R", "Q", "lam", "change", "rs", "st")], {"B": 0, "X": None}),
             (lib.ops_frame_modes_grad_f64, grad, [{"B": -1}, {"m": 0}, {"m": 3}, {"p": 9, "m": 9}, {"p": 0}, {"Nn": 1}, {"Ne": 0}]
              + [{k: None} for k in ("geo", "E", "conn", "phi", "g", "st", "gI")], {"B": 0, "geo": None})]
    for fn, args, bad, empty in cases:
        for override in bad:
            assert fn(*{**args, **override}.values()) == _cabi.ERR_INVALID_ARG, (fn.__name__, override)
        assert fn(*{**args, **empty}.values()) == _cabi.OK, fn.__name__


def test_python_entries_check_shapes_first_and_then_the_device():
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    assert {"FrameMass", "FrameModes", "frame_modes", "frame_solve_modes", "frame_modes_vjp", "differentiable_frame_frequencies"} <= set(oa.__all__)
    topo = frames.grid_frame(1, 1, device="cpu")
    for bad in (dict(mass_per_length=0.0), dict(mass_per_length=-1.0), dict(mass_per_length=np.ones(topo.Ne + 1)),
                dict(mass_per_length=1.0, kind="both"), dict(mass_per_length=1.0, nodal_mass=np.ones((topo.Nn, 2))),
                dict(mass_per_length=1.0, nodal_mass=-np.ones((topo.Nn, 3))), dict(mass_per_length=np.array([1.0, np.nan, 1.0]))):
        with pytest.raises(ValueError):
            oa.FrameMass(topo, **bad)
    mass = oa.FrameMass(topo, 157.0, np.full((topo.Nn, 3), 2000.0), kind="lumped")
    assert mass.consistent == 0 and mass.nodal_bstride == 0 and mass.d_mass.shape == (topo.Ne,) and mass.d_mass.dtype == torch.float64
    assert oa.FrameMass(topo, np.full(topo.Ne, 3.0), np.ones((4, topo.Nn, 3))).nodal_bstride == 3 * topo.Nn
    I = torch.full((2, topo.Ne), 5e-4, dtype=torch.float64)
    with pytest.raises(ValueError):
        oa.frame_solve_modes(topo, I[:, :-1], mass)
    with pytest.raises(ValueError):
        oa.frame_solve_modes(topo, I, oa.FrameMass(frames.grid_frame(1, 1, device="cpu"), 1.0))       # another topology's mass
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_solve_modes(topo, I, mass)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.differentiable_frame_frequencies(topo, I, mass)
    # on a factor: every shape before any device
    fac = frames.FrameFactor(topo, I, torch.empty(0, dtype=torch.uint8), frames._empty_solution(topo, 2, I.device))
    for bad in (dict(n_modes=0), dict(n_modes=3, n_vectors=2), dict(n_vectors=9), dict(n_vectors=7), dict(iters=0), dict(tol=0.0),
                dict(X0=torch.zeros((3, topo.Nn, 3), dtype=torch.float64)), dict(n_vectors=2, X0=torch.zeros((2, topo.Nn, 3)))):
        with pytest.raises(ValueError):
            oa.frame_modes(fac, mass, **bad)
    with pytest.raises(ValueError):
        oa.frame_modes(fac, oa.FrameMass(topo, 1.0, np.ones((3, topo.Nn, 3))))                          # per frame, for another batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_modes(fac, mass)
    shapes, st = torch.zeros((2, 2, topo.Nn, 3), dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    modes = oa.FrameModes(None, None, shapes, None, 0, st)
    with pytest.raises(ValueError):
        oa.frame_modes_vjp(fac, modes, torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_modes_vjp(fac, modes, torch.zeros((2, 2), dtype=torch.float64))
    import importlib
    fm = importlib.import_module("openpystruct_amd.frame_modes")      # (the package's attribute of that name is the function)
    assert fm.default_vectors(topo, 1) == 5 and fm.default_vectors(topo, 2) == 6 and fm.default_vectors(frames.grid_frame(3, 6, device="cpu"), 4) == 8
    np.testing.assert_array_equal(fm.default_start(topo, 3).reshape(3, -1), fr.default_start(fd.case_of(topo), 3))


def test_the_shim_records_mass_commands():
    from openpystruct_amd import ops
    ops.wipe()
    ops.model("basic", "-ndm", 2, "-ndf", 3)
    for t, xy in enumerate([(0, 0), (4, 0), (0, 3), (4, 3)], start=1):
        ops.node(t, *xy)
    ops.fix(1, 1, 1, 1); ops.fix(2, 1, 1, 1)
    ops.geomTransf("Linear", 1)
    ops.element("elasticBeamColumn", 1, 1, 3, 0.02, 200e9, 5e-4, 1)                              # as before: no mass
    ops.element("elasticBeamColumn", 2, 2, 4, 0.02, 200e9, 5e-4, 1, "-mass", 157.0)
    ops.element("elasticBeamColumn", 3, 3, 4, 0.02, 200e9, 5e-4, 1, "-mass", 80.0, "-cMass")
    ops.mass(3, 2000.0, 2000.0, 0.0)
    ops.mass(4, 1500.0, 1500.0, 10.0)
    d = ops._dom
    assert d.elements[1] == (1, 3, 0.02, 200e9, 5e-4) and d.elements[3] == (3, 4, 0.02, 200e9, 5e-4)
    assert d.ele_mass == {2: (157.0, False), 3: (80.0, True)} and d.masses == {3: (2000.0, 2000.0, 0.0), 4: (1500.0, 1500.0, 10.0)}
    with pytest.raises(NotImplementedError, match="consistent and lumped"):
        ops.eigen(1)                                                                             # mixed kinds, before any device
    ops.element("elasticBeamColumn", 2, 2, 4, 0.02, 200e9, 5e-4, 1, "-mass", 157.0, "-cMass")
    with pytest.raises(NotImplementedError, match="-mass"):
        ops.eigen("-genBandArpack", 1)                                                           # element 1 has no mass
    with ops.deferred():
        with pytest.raises(NotImplementedError, match="deferred"):
            ops.eigen(1)
    with pytest.raises(RuntimeError):
        ops.nodeEigenvector(3, 1)
    ops.wipe()
    assert ops._dom.masses == {} and ops._dom.ele_mass == {}


# ---------------------------------------------------------------------------------------------------------------------
# (d) what the GPU tests rely on, on the reference alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_conditions_of_the_gpu_cases(key):
    """Mode 1 has a relative gap of at least 0.25 to mode 2 in every frame (measured: the smallest lambda_2 / lambda_1 is about 7); the
    reference iteration reaches an eigenvalue error of 1e-10 on the compared modes within half the iterations the GPU test runs;
    mode 2 is left out of the vector and gradient comparison only where its gap to a neighbour is below 0.25."""
    ref = fr.reference(key)
    worst_gap, worst_err, skipped = np.inf, 0.0, 0
    for r in ref:
        assert fr.gap(r["lam"], 0) >= fr.GAP
        worst_gap = min(worst_gap, fr.gap(r["lam"], 0))
        lam_it = r["its"][fr.ITERS // 2 - 1][0]
        compared = [0] + ([1] if fr.gap(r["lam"], 1) >= fr.GAP else [])
        skipped += 2 - len(compared)
        for j in compared:
            worst_err = max(worst_err, abs(lam_it[j] / r["lam"][j] - 1.0))
    print(f"{key}: smallest gap of mode 1 {worst_gap:.3f}, eigenvalue error after {fr.ITERS // 2} iterations {worst_err:.2e}, mode 2 left out in {skipped} frames")
    assert worst_err <= 1e-10
