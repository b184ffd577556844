"""Linear buckling load factors on the host (no GPU): (a) the dense reference (tests/frame_buckling_ref.py) against
Euler's load of a cantilever column, and the adjoint formula of the gradient against autograd of the dense model and central
differences; (b) the arithmetic of csrc/frame_buckling.hpp -- the text the HIP kernels of csrc/frame_loads.hip compile -- built
with g++ and the address + undefined-behaviour sanitizers into a stand-alone program: geometric rows, the whole Ritz step (the 64
lanes one after the other, their partial sums added by the kernel's butterfly) and the gradient rows against the reference; (c) the
binding, the refusals of the three C entries (decided before any HIP call: no device is needed) and the argument checks of the
Python entries; (d) the conditions the GPU tests (tests/test_gpu_frame_buckling.py) rely on, on the reference alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import frame_buckling_ref as br  # noqa: E402
from tests import frame_dense as fd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpystruct_amd", "csrc")
HEADER = os.path.join(CSRC, "frame_buckling.hpp")
KEYS = list(br.CASES)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the reference itself
# ---------------------------------------------------------------------------------------------------------------------
def _column_error(n_el, kind):
    case = fd.case_of(br.column(n_el))
    I = np.full(n_el, 1e-4)
    kgu, ax = br.unit_geometric_matrices(case, kind)
    N = (br.static_forces(case, I) * ax).sum(-1)
    np.testing.assert_allclose(N, -1.0, rtol=1e-9)                   # the unit tip load, compression
    mu, _ = br.dense_buckling(case, I, br.dense_S(case, N, kgu))
    return float(br.load_factors(mu)[0] / (np.pi ** 2 * 200e9 * 1e-4 / (4 * 4.0 ** 2)) - 1.0)


def test_column_closed_form_and_order_of_convergence():
    """The first load factor of the cantilever column against pi^2 E I / (4 H^2).  Measured at 4 / 8 / 16 elements: consistent +3.3e-5,
    +2.1e-6, +1.3e-7 (order h^4); pdelta +1.3e-2, +3.2e-3, +8.0e-4 (order h^2)."""
    c = [_column_error(n, "consistent") for n in (4, 8, 16)]
    p = [_column_error(n, "pdelta") for n in (4, 8, 16)]
    print(f"consistent {c} pdelta {p}")
    assert 0.0 < c[2] < 2e-7 and 0.0 < c[0] < 5e-5
    assert 12.0 <= c[0] / c[1] <= 20.0 and 12.0 <= c[1] / c[2] <= 20.0
    assert 0.0 < p[2] < 1e-3 and 3.0 <= p[0] / p[1] <= 5.0 and 3.0 <= p[1] / p[2] <= 5.0


def formula_gradient(case, I, loads, kind, phi, lam, g):
    """sum_j g_j dlambda_j/dI by the adjoint formula of DESIGN.md §9q: the direct term plus the vector-Jacobian product of the dense
    static solve with the cotangent of the end forces that tests/frame_buckling_ref.py::grad_rows states."""
    direct, g_forces, _, _ = br.grad_rows(case, kind, phi, lam, g)
    It = torch.tensor(I, requires_grad=True)
    forces = fd.dense_frame_solve(case, It[None], None if loads is None else torch.tensor(loads))[1][0]
    return direct + torch.autograd.grad((forces * torch.tensor(g_forces)).sum(), It)[0].numpy()


@pytest.mark.parametrize("key", ["1x1-c", "3x6-p", "3x6-c", "general-c", "hub-p"])
def test_adjoint_formula_matches_autograd_and_central_differences(key):
    """Frame 0 of a shared case, both modes: the formula against autograd of the dense model through eigvalsh, norm-wise <= 1e-10
    (measured: at most 2.3e-14), and autograd against central differences with h = 1e-5 I_e on five elements, <= 1e-5 of the
    gradient's largest entry (truncation O(h^2), rounding 1e-16 / 1e-5 relative to lambda / I_e; measured: at most 1.8e-8)."""
    case, I, loads, kind, _ = br.inputs(key)
    ld = None if loads is None else loads[0]
    ref = br.reference(key)[0]
    g = np.array([0.7, -0.4])
    lam, auto = br.autograd_gradient(case, I[0], ld, kind, g)
    np.testing.assert_allclose(lam, ref["lam"][:2], rtol=1e-10)
    form = formula_gradient(case, I[0], ld, kind, ref["phi"], ref["lam"][:2], g)
    e_form = float(np.linalg.norm(form - auto) / np.linalg.norm(auto))
    e_fd = 0.0
    for e in range(0, I.shape[1], max(1, I.shape[1] // 5)):
        h = 1e-5 * I[0, e]
        up, dn = I[0].copy(), I[0].copy()
        up[e] += h; dn[e] -= h
        num = g @ (br.autograd_gradient(case, up, ld, kind, g)[0] - br.autograd_gradient(case, dn, ld, kind, g)[0]) / (2 * h)
        e_fd = max(e_fd, abs(num - auto[e]) / np.abs(auto).max())
    print(f"{key}: formula against autograd {e_form:.2e}, autograd against central differences {e_fd:.2e}")
    assert e_form <= 1e-10 and e_fd <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# (b) csrc/frame_buckling.hpp with g++
# ---------------------------------------------------------------------------------------------------------------------
_PROGRAM = r"""
#include "frame_buckling.hpp"
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
// small part, the lanes' entries of Q and R.  out: q [P,n], r [P,n], mu [P], lam [P], change [P], status, sweeps
template <int P>
static void ritz(long n, const double* x, const double* sx, std::vector<double> r, const double* prev, std::vector<double>& out) {
  constexpr int NA = FmRitz<P>::NACC;
  std::vector<double> part((size_t)FM_LANES * NA), next(part.size());
  for (int lane = 0; lane < FM_LANES; ++lane) fm_ritz_partials<P>(n, x, sx, r.data(), lane, part.data() + (size_t)lane * NA);
  for (int off = 32; off >= 1; off >>= 1) {
    for (int lane = 0; lane < FM_LANES; ++lane)
      for (int k = 0; k < NA; ++k) next[(size_t)lane * NA + k] = part[(size_t)lane * NA + k] + part[(size_t)(lane ^ off) * NA + k];
    part.swap(next);
  }
  for (int lane = 1; lane < FM_LANES; ++lane)
    for (int k = 0; k < NA; ++k)
      if (part[(size_t)lane * NA + k] != part[k] && part[k] == part[k]) { std::fprintf(stderr, "lanes differ\n"); std::exit(3); }
  double Z[P * P], mu[P], lam[P], change[P];
  int sweeps = -1;
  const int st = fb_ritz_small<P>(part.data(), prev, Z, mu, lam, change, &sweeps);
  std::vector<double> q((size_t)P * n, __builtin_nan(""));
  if (st == 0)
    for (int lane = 0; lane < FM_LANES; ++lane) fm_ritz_update<P>(n, x, sx, Z, lane, q.data(), r.data());
  out.insert(out.end(), q.begin(), q.end());
  out.insert(out.end(), r.begin(), r.end());
  for (int j = 0; j < P; ++j) out.push_back(st == 0 ? mu[j] : __builtin_nan(""));
  for (int j = 0; j < P; ++j) out.push_back(st == 0 ? lam[j] : __builtin_nan(""));
  for (int j = 0; j < P; ++j) out.push_back(st == 0 ? change[j] : __builtin_nan(""));
  out.push_back(st);
  out.push_back(sweeps);
}
// <in> <out>.  in: int32 mode (0: geometric rows, 1: Ritz, 2: gradient rows), R | B, rows_per_frame | p, Nn, Ne, consistent, m; geo, E;
// conn, ptr, idx; mode 0: forces, x; mode 1: X, SX, R, mu_prev; mode 2: phi, lambda, g
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = rd<int32_t>(f, 7);
  const int mode = h[0], R = h[1], rpf = h[2], Nn = h[3], Ne = h[4], consistent = h[5], m = h[6];
  const auto geo = rd<double>(f, 3 * (size_t)Ne), E = rd<double>(f, Ne);
  const auto conn = rd<int32_t>(f, 2 * (size_t)Ne), ptr = rd<int32_t>(f, Nn + 1), idx = rd<int32_t>(f, 2 * (size_t)Ne);
  std::vector<double> out;
  if (mode == 0) {
    const int frames = (R + rpf - 1) / rpf;
    const auto forces = rd<double>(f, (size_t)frames * Ne * 6), x = rd<double>(f, (size_t)R * Nn * 3);
    for (long r = 0; r < R; ++r)
      for (int n = 0; n < Nn; ++n) {
        double y[3];
        fb_node_geom(Nn, Ne, geo.data(), conn.data(), ptr.data(), idx.data(), forces.data(), consistent, x.data(), r, r / rpf, n, y);
        out.insert(out.end(), y, y + 3);
      }
  } else if (mode == 1) {
    const int B = R, p = rpf;
    const long n = 3L * Nn;
    const auto X = rd<double>(f, (size_t)B * p * n), SX = rd<double>(f, (size_t)B * p * n), Rr = rd<double>(f, (size_t)B * p * n);
    const auto prev = rd<double>(f, (size_t)B * p);
    for (long b = 0; b < B; ++b) {
      const double *x = X.data() + b * p * n, *sx = SX.data() + b * p * n, *pv = prev.data() + b * p;
      const std::vector<double> r(Rr.begin() + b * p * n, Rr.begin() + (b + 1) * p * n);
      switch (p) {
        case 1: ritz<1>(n, x, sx, r, pv, out); break;
        case 2: ritz<2>(n, x, sx, r, pv, out); break;
        case 3: ritz<3>(n, x, sx, r, pv, out); break;
        case 4: ritz<4>(n, x, sx, r, pv, out); break;
        case 5: ritz<5>(n, x, sx, r, pv, out); break;
        case 6: ritz<6>(n, x, sx, r, pv, out); break;
        case 7: ritz<7>(n, x, sx, r, pv, out); break;
        case 8: ritz<8>(n, x, sx, r, pv, out); break;
        default: return 2;
      }
    }
  } else {
    const int B = R, p = rpf;
    const auto phi = rd<double>(f, (size_t)B * p * Nn * 3), lam = rd<double>(f, (size_t)B * m), g = rd<double>(f, (size_t)B * m);
    for (long b = 0; b < B; ++b)
      for (int e = 0; e < Ne; ++e) {
        double d, gf[6];
        fb_elem_grad(m, p, Nn, geo.data(), E.data(), conn.data(), consistent, phi.data(), lam.data(), g.data(), b, e, &d, gf);
        out.push_back(d);
        out.insert(out.end(), gf, gf + 6);
      }
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
    assert os.path.exists(HEADER), "csrc/frame_buckling.hpp is missing"
    d = tmp_path_factory.mktemp("frame_buckling")
    src, exe = d / "frame_buckling_host.cpp", d / "frame_buckling_host"
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
    return br.topology(br.CASES[key][0], "cpu")


def _geom_ratio(program, tmp_path, key):
    """Largest elementwise |got - ref| / (2^-52 |S| |x|) of the g++ build against dense S @ x on a shared case's inputs, |S| the sum of
    the absolute terms of S (the four terms of every axial force included)."""
    case, I, _, kind, _ = br.inputs(key)
    topo, ref = _topo(key), br.reference(key)
    B = I.shape[0]
    x = br.geom_apply_x(key)
    forces = np.stack([r["forces"] for r in ref])
    y = _run(program, tmp_path, topo, [0, B * 3, 3, topo.Nn, topo.Ne, kind == "consistent", 0], [forces, x]).reshape(B, 3, -1)
    worst = 0.0
    for b in range(B):
        want, scale = x[b] @ ref[b]["S"].T, np.abs(x[b]) @ ref[b]["Sabs"].T
        worst = max(worst, float((np.abs(y[b] - want)[scale > 0] / (br.EPS * scale[scale > 0])).max()))
        assert np.all(y[b][scale == 0] == 0.0)
    return worst


def _grad_ratio(program, tmp_path, key):
    """Largest elementwise |got - ref| / (2^-52 scale) of the g++ build's gradient rows, fed the reference's phi and lambda; scale the
    sum of the absolute terms of tests/frame_buckling_ref.py::grad_rows."""
    case, I, _, kind, _ = br.inputs(key)
    topo, ref = _topo(key), br.reference(key)
    B = I.shape[0]
    phi, lam, g = np.stack([r["phi"] for r in ref]), np.stack([r["lam"][:2] for r in ref]), br.grad_cotangent(key)
    got = _run(program, tmp_path, topo, [2, B, 2, topo.Nn, topo.Ne, kind == "consistent", 2], [phi, lam, g]).reshape(B, topo.Ne, 7)
    worst = 0.0
    for b in range(B):
        d, gf, sd, sgf = br.grad_rows(case, kind, phi[b], lam[b], g[b])
        want, scale = np.concatenate([d[:, None], gf], 1), np.concatenate([sd[:, None], sgf], 1)
        worst = max(worst, float((np.abs(got[b] - want)[scale > 0] / (br.EPS * scale[scale > 0])).max()))
        assert np.all(got[b][scale == 0] == 0.0)
    return worst


@pytest.mark.parametrize("key", KEYS)
def test_host_geometric_rows_match_the_dense_matrix(program, tmp_path, key):
    """Elementwise against dense S @ x, relative to 2^-52 (|S| |x|).  Measured: at most 2.01036 (10x4n-c)."""
    worst = _geom_ratio(program, tmp_path, key)
    print(f"geometric apply: largest |got - ref| / (2^-52 |S||x|) = {worst:.5f}")
    assert worst <= br.GEOM_RATIO


@pytest.mark.parametrize("key", KEYS)
def test_host_gradient_rows_match_the_reference(program, tmp_path, key):
    """Fed the reference's phi and lambda: the direct term and the six cotangents of the end forces, elementwise relative to 2^-52
    times the sum of their absolute terms.  Measured: at most 3.67196 (10x4n-c)."""
    worst = _grad_ratio(program, tmp_path, key)
    print(f"gradient rows: largest |got - ref| / (2^-52 scale) = {worst:.5f}")
    assert worst <= br.BGRAD_RATIO


def test_the_gpu_constants_are_four_times_the_largest_host_ratio(program, tmp_path):
    """C_GEOM and C_BGRAD of tests/frame_buckling_ref.py, the constants of the elementwise GPU bounds, are 4 x the largest ratio this
    build shows over all shared cases, the ratio written down to two decimals (rounded up): pinned from below and from above."""
    geom = max(_geom_ratio(program, tmp_path, key) for key in KEYS)
    grad = max(_grad_ratio(program, tmp_path, key) for key in KEYS)
    print(f"largest ratios: geometric apply {geom:.5f}, gradient rows {grad:.5f}")
    assert br.GEOM_RATIO - 0.01 < geom <= br.GEOM_RATIO and br.BGRAD_RATIO - 0.01 < grad <= br.BGRAD_RATIO
    assert br.C_GEOM == 4.0 * br.GEOM_RATIO and br.C_BGRAD == 4.0 * br.BGRAD_RATIO


def test_host_gradient_rows_skip_an_infinite_load_factor(program, tmp_path):
    """A mode with lambda = +inf contributes nothing: the rows with (lambda_1, +inf) equal, bit for bit, the rows of mode 1 alone."""
    key = "general-c"
    topo, ref = _topo(key), br.reference(key)
    phi, lam, g = ref[0]["phi"][None], ref[0]["lam"][None, :2].copy(), br.grad_cotangent(key)[:1]
    lam[0, 1] = np.inf
    both = _run(program, tmp_path, topo, [2, 1, 2, topo.Nn, topo.Ne, 1, 2], [phi, lam, g])
    one = _run(program, tmp_path, topo, [2, 1, 2, topo.Nn, topo.Ne, 1, 1], [phi, lam[:, :1], g[:, :1]])
    assert np.array_equal(both, one) and np.all(np.isfinite(both))


def _ritz_fields(out, p, n):
    q, r = out[:p * n].reshape(p, n), out[p * n:2 * p * n].reshape(p, n)
    mu, lam, change = (out[2 * p * n + k * p:2 * p * n + (k + 1) * p] for k in range(3))
    return q, r, mu, lam, change, out[-2], out[-1]


SWEEPS = {}          # (key, p) -> the largest Jacobi sweep count the program reported
INDEFINITE = {("3x6-p", 8), ("3x6-c", 8), ("hub-p", 5), ("hub-p", 8)}      # steps whose Sr has Ritz values of both signs


@pytest.mark.parametrize("p", [1, 2, 5, 8])
@pytest.mark.parametrize("key", KEYS)
def test_host_ritz_step_matches_the_reference_iteration(program, tmp_path, key, p):
    """The whole Ritz step of iterations 1, 2 and 3 of the reference iteration on p vectors (the 1 x 1 frame: at most 3), fed the
    reference's X, SX and R: Ritz values <= 1e-10 of the largest |mu| of the step (Sr has Ritz values of both signs in the steps
    INDEFINITE names: a small mu between a positive and a negative one is a difference of large terms), descending; lambda = 1 / mu
    where mu > 0, else +inf, bit for bit; Q^T K Q = I (bound in the body); the next R = S Q; the Jacobi loop short of its cap, its
    sweep count recorded in SWEEPS; change = |mu - prev| / |mu| bit for bit.
    Measured: Ritz values at most 7.2e-14 (hub-p, eight vectors), Q^T K Q - I at most 3.81 x 2^-52 max(|Q|^T |K| |Q|) (general-c, eight
    vectors), at most 6 sweeps.  1e-10 is the figure below which the GPU tests use the project's 1e-8."""
    case, I, loads, kind, _ = br.inputs(key)
    topo, ref = _topo(key), br.reference(key)
    p = min(p, 3) if key.startswith("1x1") else p
    B = min(I.shape[0], 3)
    n = 3 * topo.Nn
    its = [br.iterate(case, I[b], ref[b]["S"], br.default_start(case, p), 3) for b in range(B)]
    worst, worst_orth, indefinite = 0.0, 0.0, False
    for t in range(3):
        X, SX, R = (np.stack([its[b][t][k] for b in range(B)]) for k in (3, 4, 5))
        prev = np.stack([its[b][t - 1][0] if t else np.full(p, np.inf) for b in range(B)])
        out = _run(program, tmp_path, topo, [1, B, p, topo.Nn, topo.Ne, 0, 0], [X, SX, R, prev]).reshape(B, -1)
        for b in range(B):
            q, r, mu, lam, change, st, sweeps = _ritz_fields(out[b], p, n)
            want = its[b][t][0]
            assert st == 0 and 0 <= sweeps < 16, (t, b, st, sweeps)
            SWEEPS[key, p] = max(SWEEPS.get((key, p), 0), int(sweeps))
            indefinite |= bool(want.min() < 0.0 < want.max())
            e_mu = float(np.abs(mu - want).max() / np.abs(want).max())
            K = br.dense_K(case, I[b])
            e_orth = float(np.abs(q @ K @ q.T - np.eye(p)).max())
            e_r = float(np.linalg.norm(r - q @ ref[b]["S"].T) / np.linalg.norm(r))
            worst = max(worst, e_mu)
            print(f"t {t + 1} frame {b}: mu {e_mu:.2e} orth {e_orth:.2e} R {e_r:.2e} sweeps {int(sweeps)}")
            assert e_mu <= 1e-10 and e_r <= 1e-12 and np.all(np.diff(mu) <= 0.0)
            # Q^T K Q = Z^T Kr Z: Z from a Cholesky factor of Kr (p eps cond(Kr)), Kr and this check's own product sums of terms of
            # both signs (K has entries of 1e9 against displacements of 1e-5), each good to a few eps of the sum of its absolute terms
            scale = float((np.abs(q) @ np.abs(K) @ np.abs(q).T).max())
            worst_orth = max(worst_orth, e_orth / (br.EPS * scale))
            assert e_orth <= br.EPS * (p * float(np.linalg.cond(its[b][t][6])) + 16.0 * scale), (e_orth, scale)
            assert np.array_equal(lam, br.load_factors(mu)) and np.all(lam > 0.0)
            assert np.array_equal(change, np.abs(mu - prev[b]) / np.abs(mu)) and (t > 0 or np.all(np.isinf(change)))
    print(f"{key} p {p}: Ritz values {worst:.2e}, orthonormality / (2^-52 |Q|^T |K| |Q|) {worst_orth:.2f}, sweeps {SWEEPS[key, p]}, indefinite Sr {indefinite}")
    assert indefinite or (key, p) not in INDEFINITE


def test_host_ritz_step_reports_a_pencil_that_is_not_positive_definite(program, tmp_path):
    """pdelta on the 1 x 1 frame: every element carries one transverse difference, so S has rank three; five vectors, and four (rank +
    1: the fourth pivot is rounding noise of either sign, which FB_MIN_PIVOT catches and `d > 0` would not in half the draws), give
    status 2, NaN and an untouched R; three are served."""
    case = fd.case_of(br.topology("1x1", "cpu"))
    topo = br.topology("1x1", "cpu")
    I = br.inputs("1x1-c")[1][0]
    kgu, ax = br.unit_geometric_matrices(case, "pdelta")
    S = br.dense_S(case, (br.static_forces(case, I) * ax).sum(-1), kgu)
    f = br.free_dofs(case)
    n = 3 * topo.Nn
    for p, want in ((5, 2.0), (4, 2.0), (3, 0.0)):
        R = br.default_start(case, p) @ S.T
        X = np.zeros_like(R)
        X[:, f] = np.linalg.solve(br.dense_K(case, I)[np.ix_(f, f)], R[:, f].T).T
        out = _run(program, tmp_path, topo, [1, 1, p, topo.Nn, topo.Ne, 0, 0], [X, X @ S.T, R, np.full(p, np.inf)])
        q, r, mu, lam, change, st, _ = _ritz_fields(out, p, n)
        assert st == want
        assert bool(np.isnan(q).all()) == bool(np.isnan(np.concatenate([mu, lam, change])).all()) == (want != 0.0)
        if want:
            assert np.array_equal(r, R)          # R stays


def test_host_ritz_step_gives_infinite_load_factors_under_tension(program, tmp_path):
    """The 4-element column under tip tension: every Ritz value is negative, every load factor +inf, status 0."""
    topo = br.column(4, load=+1.0)
    case = fd.case_of(topo)
    I = np.full(4, 1e-4)
    kgu, ax = br.unit_geometric_matrices(case, "consistent")
    S = br.dense_S(case, (br.static_forces(case, I) * ax).sum(-1), kgu)
    it = br.iterate(case, I, S, br.default_start(case, 5), 1)[0]
    out = _run(program, tmp_path, topo, [1, 1, 5, topo.Nn, topo.Ne, 0, 0], [it[3], it[4], it[5], np.full(5, np.inf)])
    q, r, mu, lam, change, st, _ = _ritz_fields(out, 5, 3 * topo.Nn)
    assert st == 0 and np.all(mu < 0.0) and np.all(np.isinf(lam)) and np.all(lam > 0.0) and np.all(np.diff(mu) <= 0.0)
    np.testing.assert_allclose(mu, it[0], rtol=1e-10)


# ---------------------------------------------------------------------------------------------------------------------
# (c) binding, refusals, argument checks
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = {"ops_frame_geom_apply_f64", "ops_frame_buckling_ritz_f64", "ops_frame_buckling_grad_f64"}


def test_the_entries_are_extension_exports_and_the_file_counts_hold():
    from openpystruct_amd import _cabi, build
    assert ENTRIES <= set(_cabi.EXTENSION_EXPORTS) and not ENTRIES & set(_cabi.EXPORTS)
    ext = _cabi._extensions[os.path.join(ROOT, "include", "openpystruct_amd_frame_loads.h")]
    assert ENTRIES <= set(ext.functions)
    assert len(build.SOURCES) == 26 and len(_cabi.EXTENSION_HEADER_PATHS) == 9 and len(_cabi.EXPORTS) == 70
    deps = {os.path.basename(p) for p in build._deps(os.path.join(CSRC, "frame_loads.hip"))}
    assert {"frame_buckling.hpp", "frame_modes.hpp", "frame_adjoint.hpp"} <= deps


def test_c_entries_refuse_bad_arguments_without_a_device():
    """Every refusal is decided before any HIP call, so the codes come back on a machine without a GPU; the pointers are never read."""
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    x = 1 << 20                                                     # a non-NULL address that is never dereferenced
    geom = dict(R=6, rpf=2, Nn=4, Ne=3, geo=x, conn=x, ptr=x, idx=x, forces=x, consistent=1, x=x, y=x, stream=None)
    ritz = dict(B=3, p=2, Nn=4, X=x, SX=x, R=x, Q=x, mu=x, lam=x, change=x, rs=x, st=x, stream=None)
    grad = dict(B=3, m=2, p=2, Nn=4, Ne=3, geo=x, E=x, conn=x, consistent=0, phi=x, lam=x, g=x, st=x, gI=x, gf=x, stream=None)
    cases = [(lib.ops_frame_geom_apply_f64, geom, [{"R": -1}, {"rpf": 0}, {"Nn": 1}, {"Nn": -4}, {"Ne": 0}]
              + [{k: None} for k in ("geo", "conn", "ptr", "idx", "forces", "x", "y")], {"R": 0, "geo": None}),
             (lib.ops_frame_buckling_ritz_f64, ritz, [{"B": -1}, {"p": 0}, {"p": 9}, {"p": -2}, {"Nn": 1}]
              + [{k: None} for k in ("X", "SX", "R", "Q", "mu", "lam", "change", "rs", "st")], {"B": 0, "X": None}),
             (lib.ops_frame_buckling_grad_f64, grad, [{"B": -1}, {"m": 0}, {"m": 3}, {"p": 9, "m": 9}, {"p": 0}, {"Nn": 1}, {"Ne": 0}]
              + [{k: None} for k in ("geo", "E", "conn", "phi", "lam", "g", "st", "gI", "gf")], {"B": 0, "geo": None})]
    for fn, args, bad, empty in cases:
        for override in bad:
            assert fn(*{**args, **override}.values()) == _cabi.ERR_INVALID_ARG, (fn.__name__, override)
        assert fn(*{**args, **empty}.values()) == _cabi.OK, fn.__name__


def test_python_entries_check_shapes_first_and_then_the_device():
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    assert {"FrameBuckling", "frame_buckling", "frame_solve_buckling", "frame_buckling_vjp", "differentiable_frame_buckling"} <= set(oa.__all__)
    topo = frames.grid_frame(1, 1, device="cpu")
    I = torch.full((2, topo.Ne), 5e-4, dtype=torch.float64)
    with pytest.raises(ValueError):
        oa.frame_solve_buckling(topo, I[:, :-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_solve_buckling(topo, I)
    with pytest.raises(ValueError):
        oa.differentiable_frame_buckling(topo, I, kind="both")
    with pytest.raises(ValueError):
        oa.differentiable_frame_buckling(topo, I[:, :-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.differentiable_frame_buckling(topo, I)
    # on a factor: every shape before any device
    sol = frames._empty_solution(topo, 2, I.device)
    fac = frames.FrameFactor(topo, I, torch.empty(0, dtype=torch.uint8), sol)
    other = frames._empty_solution(topo, 3, I.device)
    for bad in (dict(n_modes=0), dict(n_modes=3, n_vectors=2), dict(n_vectors=9), dict(n_vectors=7), dict(iters=0), dict(tol=0.0), dict(kind="lumped"),
                dict(X0=torch.zeros((3, topo.Nn, 3), dtype=torch.float64)), dict(n_vectors=2, X0=torch.zeros((2, topo.Nn, 3))),
                dict(reference=other), dict(reference=sol.forces), dict(reference=frames.FrameSolution(sol.disp, sol.forces.float(), sol.V, sol.M, sol.status))):
        with pytest.raises(ValueError):
            oa.frame_buckling(fac, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_buckling(fac)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_buckling(fac, reference=sol, kind="pdelta", n_vectors=3)
    shapes, st, lam = torch.zeros((2, 2, topo.Nn, 3), dtype=torch.float64), torch.zeros(2, dtype=torch.int32), torch.ones((2, 2), dtype=torch.float64)
    res = oa.FrameBuckling(lam, None, shapes, None, 0, st, sol, "consistent")
    with pytest.raises(ValueError):
        oa.frame_buckling_vjp(fac, res, torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        oa.frame_buckling_vjp(fac, res._replace(kind="lumped"), torch.zeros((2, 2), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_buckling_vjp(fac, res, torch.zeros((2, 2), dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# (d) what the GPU tests rely on, on the reference alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_conditions_of_the_gpu_cases(key):
    """For every frame of every case the NumPy restatement of the iteration reaches |mu - mu_dense| / |mu_dense| <= 1e-10 on the two
    compared modes within the 16 iterations the GPU test runs, both modes buckle (mu > 0) and X^T K X stays positive definite (the
    restatement's Cholesky factorisation would raise) with a condition number far from 2^52.  Its shapes, in the K-norm x min(1, gap)
    on the compared modes (mode 2 where its gap is at least 0.25), are within 1e-10 of the dense ones or within the figure
    tests/frame_buckling_ref.py::SHAPE_ERROR records for the case, from which the GPU bound follows.
    Measured: mu at most 2.0e-15, cond(X^T K X) at most 2.3e4 (hub-p), shapes 1.1e-9 (3x6-c), 1.1e-8 (10x4n-c), else at most 2e-14."""
    case, I = br.inputs(key)[:2]
    ref = br.reference(key)
    worst, cond, shape, gap1, gap2 = [0.0, 0.0], 0.0, 0.0, np.inf, np.inf
    for b, r in enumerate(ref):
        assert r["mu"][0] > 0.0 and r["mu"][1] > 0.0
        mu_it, Q = r["its"][br.ITERS - 1][0], br.fix_sign(r["its"][br.ITERS - 1][1])
        K = br.dense_K(case, I[b])
        for j in (0, 1):
            worst[j] = max(worst[j], abs(mu_it[j] - r["mu"][j]) / abs(r["mu"][j]))
            if j == 0 or br.gap(r["mu"], 1) >= br.GAP:
                shape = max(shape, br.shape_error(K, Q[j], r["phi"][j]) * min(1.0, br.gap(r["mu"], j)))
        cond = max(cond, max(float(np.linalg.cond(it[6])) for it in r["its"]))
        gap1, gap2 = min(gap1, br.gap(r["mu"], 0)), min(gap2, br.gap(r["mu"], 1))
    print(f"{key}: mu error after {br.ITERS} iterations {worst[0]:.2e} {worst[1]:.2e}, shapes {shape:.3e}, cond(Kr) {cond:.2e}, smallest gaps {gap1:.3f} {gap2:.3f}")
    assert max(worst) <= 1e-10 and cond <= 1e8
    if key in br.SHAPE_ERROR:
        assert 0.5 * br.SHAPE_ERROR[key] < shape <= br.SHAPE_ERROR[key] and br.shape_bound(key) == 100.0 * br.SHAPE_ERROR[key]
    else:
        assert shape <= 1e-10 and br.shape_bound(key) == 1e-8
