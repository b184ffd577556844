"""The C-ABI shared library loads on a machine without a GPU and exports every symbol
include/openpystruct_amd.h declares (no compute calls here)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from openpystruct_amd import _cabi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _cabi.load()


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "openpystruct_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ops_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_cabi.EXPORTS) and len(_cabi.EXPORTS) == len(declared)
    for name in declared:
        assert getattr(lib, name) is not None
        assert getattr(lib, name).argtypes is not None, name        # every entry point is called with checked argument types


def test_abi_version(lib):
    assert lib.ops_amd_abi_version() == 14 == _cabi.ABI_VERSION     # 14: ops_tfd_head_bwd_args.ln_part; 13: ops_frame_solve_batched_f64_ex (OPS_FRAME_REUSE_PLAN), ops_frame_plan_signature; 12: ops_mlp_wgrad_group_norm, OPS_ADAM_NORM_READY; 11: ops_tfd_front_args.n_order (a walked-past cursor wraps); 10: loss on the TFD head's tile, identity_act of the TFD launches, ops_physics_loss_*; 2: ops_beam_sizing_epoch_f32 takes I_last (float32) instead of I64; 3: ops_mlp_* layer blocks; 4: diffusion combine with a bf16 copy / two gradients; 5: encoder-layer launches on tiled weights; 6: head / front-end launches, column-sum jobs and 24 problems in the grouped weight-gradient launch, ln_part; 7: ops_mlp_strip_args.eval_stats; 8: ops_sizing_draw_cases_f64; 9: evaluation slots of ops_mlp_strip_args


_REFEREE = r"""
#include "openpystruct_amd.h"
#include <cstddef>
#include <cstdio>
#include <type_traits>
template <class T> void kind() {        // " <sizeof>:<p|f|s|u>" (pointer, floating, signed, unsigned), " 0:v" for void
  if constexpr (std::is_void_v<T>) std::printf(" 0:v");
  else std::printf(" %zu:%c", sizeof(T), std::is_pointer_v<T> ? 'p' : std::is_floating_point_v<T> ? 'f' : std::is_signed_v<T> ? 's' : 'u');
}
template <class R, class... A> void sig(const char* name, R (*)(A...)) {
  std::printf("F %s", name); kind<R>(); (kind<A>(), ...); std::printf("\n");
}
#define STRUCT(S) std::printf("S %s %zu\n", #S, sizeof(S))
#define FIELD(S, f) (std::printf("M %s %s %zu", #S, #f, offsetof(S, f)), kind<decltype(S::f)>(), std::printf("\n"))
#define FUNC(f) sig(#f, static_cast<decltype(&f)>(nullptr))      /* the type only: nothing to link against */
int main() {
@CALLS@  return 0;
}
"""


def _kind(t) -> str:
    """What the referee prints for a C type, for the ctypes type the binding chose."""
    if t is None:
        return "0:v"
    code = t._type_ if isinstance(getattr(t, "_type_", None), str) else "P"          # POINTER(...): _type_ is the pointee class
    return f"{ctypes.sizeof(t)}:{'p' if code in 'Pz' else 'f' if code in 'fd' else 's' if code.islower() else 'u'}"


def test_binding_agrees_with_the_compiler(tmp_path):
    """The compiler is the referee of the header reader: a C++ program that includes the real header reports sizeof / offsetof / kind
    of every struct field and the arity, widths and kinds of every prototype; the ctypes Structures and argtypes must say the same."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found: the referee program cannot be built")
    abi = _cabi._abi
    lines = []
    for name, cls in abi.structs.items():
        lines.append(f"  STRUCT({name});\n")
        lines += [f"  FIELD({name}, {field});\n" for field, _ in cls._fields_]
    lines += [f"  FUNC({name});\n" for name in abi.functions]
    src, exe = tmp_path / "referee.cpp", tmp_path / "referee"
    src.write_text(_REFEREE.replace("@CALLS@", "".join(lines)))
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes, members, functions = {}, {}, {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        tag, name, *rest = line.split()
        if tag == "S":
            sizes[name] = int(rest[0])
        elif tag == "M":
            members[name, rest[0]] = (int(rest[1]), rest[2])
        else:
            functions[name] = rest
    assert len(sizes) == len(abi.structs) == 14 and len(functions) == len(abi.functions) == 70
    for name, cls in abi.structs.items():
        assert getattr(_cabi, cls.__name__) is cls, f"struct {name} has no line {cls.__name__} = _struct(...) in _cabi.py"
        assert ctypes.sizeof(cls) == sizes[name], f"struct {name}: ctypes {ctypes.sizeof(cls)} bytes, compiler {sizes[name]}"
        for field, t in cls._fields_:
            assert (getattr(cls, field).offset, _kind(t)) == members[name, field], f"struct {name}.{field}"
    for name, (restype, argtypes) in abi.functions.items():
        assert [_kind(restype)] + [_kind(t) for t in argtypes] == functions[name], f"function {name}"


_ACCEPTED = """
/* a header of the shape of the real one */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define OPS_AMD_ONE 1u   /* unsigned suffix */
#define OPS_HEX 0x200
#define OPS_PLAIN 24
typedef struct ops_pair {
  float a, b;                       /* two declarators */
  /* a comment between fields */
  const float* const* p; int32_t n; // two declarations on one line
  double *x, y;
  unsigned long long seed; long long* rows; int64_t stride;
} ops_pair;
int ops_one(int n, const ops_pair* args, const ops_pair* const* list, void* stream); size_t ops_two(void);
const char* ops_name(const char* key, long value, unsigned flags);
void ops_fill(const uint8_t* mask,
              float* out /* [n] */);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_reader_reads_the_forms_the_header_uses():
    c = ctypes
    abi = _cabi.read_header(_ACCEPTED)
    assert abi.defines == {"OPS_AMD_ONE": 1, "OPS_HEX": 0x200, "OPS_PLAIN": 24}
    pair = abi.structs["ops_pair"]
    assert list(abi.structs) == ["ops_pair"] and pair.__name__ == "Pair"
    assert pair._fields_ == [("a", c.c_float), ("b", c.c_float), ("p", c.c_void_p), ("n", c.c_int32), ("x", c.c_void_p), ("y", c.c_double),
                             ("seed", c.c_ulonglong), ("rows", c.c_void_p), ("stride", c.c_int64)]
    assert pair(a=1.5, n=3).n == 3 and c.sizeof(pair) == 64
    assert abi.functions == {"ops_one": (c.c_int, [c.c_int, c.POINTER(pair), c.c_void_p, c.c_void_p]), "ops_two": (c.c_size_t, []),
                             "ops_name": (c.c_char_p, [c.c_char_p, c.c_long, c.c_uint]), "ops_fill": (None, [c.c_void_p, c.c_void_p])}


@pytest.mark.parametrize("text, complaint", [
    ("typedef struct ops_a { float w[4]; } ops_a;", "w[4]"),                                        # array member
    ("typedef struct ops_a { int32_t flag : 1; } ops_a;", "flag : 1"),                                # bit field
    ("typedef struct ops_a { int n; } ops_a;\ntypedef struct ops_b { ops_a inner; } ops_b;", "'ops_a' by value"),
    ("typedef struct ops_a { int n; } ops_a;\nint ops_f(ops_a a);", "'ops_a' by value"),
    ("typedef struct ops_a { struct { int n; } in; } ops_a;", "typedef struct ops_a"),               # nested struct
    ("struct ops_a { int n; };", "struct ops_a"),                                                    # not the typedef form
    ("typedef struct ops_a { int n; } ops_b;", "ops_b"),
    ("int ops_f(void (*callback)(int), void* stream);", "int ops_f"),                                # function-pointer parameter
    ("int ops_f(uint16_t n);", "unknown type 'uint16_t'"),
    ("int ops_f(unsigned long n);", "unknown type 'unsigned long'"),
    ("short ops_f(int n);", "unknown type 'short'"),
    ("typedef struct ops_a { ops_later* p; } ops_a;", "unknown type 'ops_later'"),
    ("int ops_f(int);", "no name"),
    ("int ops_f();", "ops_f"),
    ("int ops_f(int n);\nstatic int counter;\nint ops_g(int n);", "static int counter"),            # stray text between declarations
    ("int ops_f(int n) int ops_g(int n);", "int ops_f"),                                             # unsplittable prototype
    ("int ops_f(int n);\nint ops_f(int n);", "declared twice"),
    ("int ops_f(int n = 3);", "n = 3"),
    ("#define OPS_SHIFT (1 << 4)\n", "OPS_SHIFT"),
    ("#define OPS_PI 3.14\n", "OPS_PI"),
    ("#define OPS_MAX(a, b) 1\n", "OPS_MAX"),
    ("#define OPS_LONG 1 \\\n + 2\n", "continuation"),
])
def test_header_reader_refuses_what_it_cannot_read(text, complaint):
    """A declaration the reader skipped would be an entry point driven without checked types: everything it does not understand is an error."""
    with pytest.raises(ValueError) as e:
        _cabi.read_header(text)
    assert complaint in str(e.value)


def test_missing_header_is_reported_with_its_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_cabi, "HEADER_PATH", str(tmp_path / "nowhere.h"))
    with pytest.raises(_cabi.ExtensionMissingError, match="nowhere.h"):
        _cabi._read_abi()


def test_check_turns_a_return_code_into_an_exception(lib):
    assert _cabi.check(_cabi.OK, "ops_something") is None
    z = ctypes.c_void_p(0)
    rc = lib.ops_beam_solve_batched_f64(-1, 100, z, 0, z, 0, z, 100, z, 0, z, 101, z, 0, z, z, z, z, z, 0, z)
    with pytest.raises(RuntimeError, match=r"^ops_beam_solve_batched_f64 failed with code 1(: .+)?$"):
        _cabi.check(rc, "ops_beam_solve_batched_f64")


def test_size_and_kernel_name_introspection(lib):
    assert lib.ops_amd_max_elements() >= 100
    assert b"beam_rows_kernel<16, 7" in lib.ops_beam_solve_kernel_name(10000, 100, 0)       # default: the row-staged 16-lane kernel
    assert b"beam_rows_kernel<16, 7" in lib.ops_beam_solve_kernel_name(100000, 100, 0)
    assert b"beam_solve_kernel<8, 13" in lib.ops_beam_solve_kernel_name(1 << 20, 100, 0)   # bandwidth-bound batches: flat aligned streams
    assert b"beam_solve_kernel<16, 7" in lib.ops_beam_solve_kernel_name(10000, 100, 16)     # explicit P without OPS_AMD_TILING_ROWS: beam_solve.hip
    assert b"beam_solve_kernel<32, 4" in lib.ops_beam_solve_kernel_name(10000, 120, 0)      # beyond 16 x 7 nodes: beam_solve.hip
    assert b"beam_rows_kernel<6, 17" in lib.ops_beam_solve_kernel_name(64, 100, 6)          # the fat-wave tiling (csrc/beam_fat.hip)
    assert b"beam_rows_kernel<16, 7" in lib.ops_beam_solve_kernel_name(64, 100, 16 | 0x200)  # OPS_AMD_TILING_ROWS
    assert lib.ops_beam_solve_kernel_name(64, 300, 6) == b""
    assert lib.ops_beam_solve_kernel_name(10, 5000, 0) == b""


def test_argument_validation_without_gpu(lib):
    # invalid arguments are rejected before any HIP call
    z = ctypes.c_void_p(0)
    rc = lib.ops_beam_solve_batched_f64(4, 100, z, 0, z, 0, z, 100, z, 0, z, 101, z, 0, z, z, z, z, z, 0, z)
    assert rc == _cabi.ERR_INVALID_ARG
    rc = lib.ops_beam_solve_batched_f64(-1, 100, z, 0, z, 0, z, 100, z, 0, z, 101, z, 0, z, z, z, z, z, 0, z)
    assert rc == _cabi.ERR_INVALID_ARG
    rc = lib.ops_beam_solve_batched_f64(0, 100, z, 0, z, 0, z, 100, z, 0, z, 101, z, 0, z, z, z, z, z, 0, z)
    assert rc == _cabi.OK   # empty batch is a no-op
    # the other entry points: NULL pointers / bad sizes are refused the same way
    hp = _cabi.SizingParams(E=2e11, G=7.7e10, alpha_moment=1e-2, alpha_shear=1e-2, lr=0.01, gamma=0.98, beta1=0.9, beta2=0.999,
                            adam_eps=1e-8, clamp_min=1e-8, bend_eps=1e-6, area_coef=0.03, tolerance=5e-3, patience=5, max_epochs=10)
    assert lib.ops_beam_solve_forces_f64(4, 100, z, 0, z, 0, z, 100, z, 0, z, 101, z, 0, z, z, z, z, 0, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_beam_solve_forces_f32(4, 100, z, 0, z, 0, z, 100, z, 0, z, 101, z, 0, z, z, z, z, 0, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_beam_sizing_step_f32(4, 100, *([z] * 13), ctypes.byref(hp), z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_beam_sizing_step_f32(4, 600, *([z] * 13), ctypes.byref(hp), z) == _cabi.ERR_UNSUPPORTED
    assert lib.ops_beam_sizing_step_vm32_f32(4, 100, *([z] * 11), ctypes.byref(hp), z, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_beam_sizing_epoch_f32(4, 100, z, 0, z, 0, z, 0, z, 101, z, 0, *([z] * 9), ctypes.byref(hp), z, z, 0, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_beam_sizing_epoch_f32(4, 200, z, 0, z, 0, z, 0, z, 201, z, 0, *([z] * 9), ctypes.byref(hp), z, z, 0, z) == _cabi.ERR_UNSUPPORTED
    assert lib.ops_frame_solve_batched_f64(2, 4, 3, 6, 5, *([z] * 8), 0, *([z] * 6), 0, z) == _cabi.ERR_INVALID_ARG
    # large batches keep the factor in the caller's workspace: one column-major L per frame (window width 36 / 52 for these bands) + the plan;
    # a frame whose band does not fit LDS needs the workspace at any batch (15 x 16: band + rhs per frame)
    assert lib.ops_frame_workspace_bytes(5000, 330, 35) >= 5000 * 330 * 36 * 8 and lib.ops_frame_workspace_bytes(3, 768, 50) >= 3 * 768 * 53 * 8
    assert lib.ops_frame_workspace_bytes(40000, 90, 17) >= 40000 * 90 * 18 * 8      # packed kernel (half bandwidth <= 29): window width 18
    assert lib.ops_frame_plan_signature(40000, 90, 17) >> 24 == 2 and lib.ops_frame_plan_signature(5000, 330, 35) >> 24 == 1 and lib.ops_frame_plan_signature(3, 330, 35) == 0
    assert lib.ops_amd_get_option(b"frame_pack") == 1 and lib.ops_amd_get_option(b"frame_latency_batch") == -1 and lib.ops_amd_get_option(b"nope") == -2
    assert lib.ops_amd_get_option(b"frame_coop") == 1 and lib.ops_amd_set_option(b"frame_coop", 3) != _cabi.OK
    assert lib.ops_amd_set_option(b"nope", 1) == _cabi.ERR_INVALID_ARG
    assert lib.ops_frame_workspace_bytes(3, 330, 35) == 0        # r05: small batches (<= 256 .. 4 000 frames by size) whose band fits LDS take the workgroup-per-frame kernels
    assert lib.ops_frame_workspace_bytes(0, 330, 35) == 0
    assert lib.ops_stencil3_bn1_fwd_f32(2, 3, z, z, z, z, z, 1e-5, 0.1, 1, z, z, z, z, 0, z, z, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_stencil3_bn1_bwd_f32(2, 3, z, z, 0, z, z, z, z, 1, z, z, z, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_flat_clip_adam_step_f32(10, z, z, z, z, z, z, 1.0, 1.0, 0.9, 0.999, 1e-8, 0.0, 0, z, z, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_surrogate_loss_grad_f32(2, 3, 3, 0, z, 0, z, z, 0.5, z, z, 0.1, 0.0, z, z, z, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_beam_residual_f64(2, 3, *([z, 0] * 2), z, z, 0, z, z, 0, z, z, z, z, z) == _cabi.ERR_INVALID_ARG
    # layer blocks of the PINN step: broken layout contracts are refused on the host
    a = _cabi.MlpStripArgs()
    assert lib.ops_mlp_strip_launch(None, z) == _cabi.ERR_INVALID_ARG and lib.ops_mlp_strip_launch(a, z) == _cabi.ERR_INVALID_ARG
    a.B, a.N, a.K, a.A, a.lda, a.W, a.ldw, a.Y, a.ldy = 129, 16, 32, 64, 32, 64, 32, 64, 32
    assert lib.ops_mlp_strip_launch(a, z) == _cabi.ERR_INVALID_ARG       # more rows than a workgroup owns
    a.B, a.lda = 128, 24
    assert lib.ops_mlp_strip_launch(a, z) == _cabi.ERR_INVALID_ARG       # reduction not padded to whole 32-column steps
    assert lib.ops_mlp_spart_doubles(350) == 44 * 12
    assert lib.ops_mlp_wgrad_group(0, None, z) == _cabi.ERR_INVALID_ARG and lib.ops_mlp_wgrad_group(9, (_cabi.MlpWgradProblem * 9)(), z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_mlp_repack_weights(1, (_cabi.MlpRepackEntry * 1)(), z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_mlp_gather_noise(200, 684, z, z, z, 1, z, z, 704, z, z, 0, z, z) == _cabi.ERR_INVALID_ARG
    assert lib.ops_mlp_loss_workspace_bytes() > 0
    sched = (ctypes.c_float * 20)()
    lib.ops_sizing_schedule_f32(ctypes.byref(hp), ctypes.cast(sched, ctypes.c_void_p))       # host-only helper
    assert sched[0] == pytest.approx(0.01 / (1 - 0.9), rel=1e-6) and sched[1] == pytest.approx((1 - 0.999) ** 0.5, rel=1e-6)
    assert sched[2] == pytest.approx(0.01 * 0.98 / (1 - 0.81), rel=1e-6)
    # case draws of the generator: counts beyond the eight pick slots, too few nodes, missing outputs
    draw = lambda B, N, R, F, rb, nf, out: lib.ops_sizing_draw_cases_f64(B, 0, 1, N, R, F, rb, z, nf, 15.0, 200.0, -1e6, -1e4, *([out] * 8), z)   # noqa: E731
    assert draw(4, 101, 4, 9, 1, 0, 64) == _cabi.ERR_INVALID_ARG and draw(4, 101, 9, 4, 1, 0, 64) == _cabi.ERR_INVALID_ARG
    assert draw(4, 3, 1, 1, 1, 0, 64) == _cabi.ERR_INVALID_ARG and draw(4, 101, 4, 4, 0, 3, 64) == _cabi.ERR_INVALID_ARG      # fixed rollers without their array
    assert draw(4, 101, 4, 4, 1, 0, z) == _cabi.ERR_INVALID_ARG and draw(0, 101, 4, 4, 1, 0, z) == _cabi.OK


def test_no_cpu_fallback():
    import torch

    import openpystruct_amd as oa

    I = torch.full((2, 10), 0.1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.beam_solve(torch.linspace(0, 1, 11, dtype=torch.float64), 2e11, I, torch.zeros(11, dtype=torch.uint8),
                      torch.zeros(2, 11, dtype=torch.float64), 0.0)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "openpystruct_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                src = open(os.path.join(dp, fn)).read()
                assert "import oracle" not in src and "from oracle" not in src and "oracle/" not in src, fn


def test_torch_library_op_is_registered_gpu_only():
    import torch
    import openpystruct_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.openpystruct_amd.beam_solve
    with FakeTensorMode():
        I = torch.empty(7, 100, dtype=torch.float64)
        v, th, V, M, st = op(torch.empty(101, dtype=torch.float64), torch.empty((), dtype=torch.float64), I,
                             torch.empty(101, dtype=torch.uint8), torch.empty(7, 101, dtype=torch.float64),
                             torch.empty((), dtype=torch.float64))
    assert v.shape == (7, 101) and th.shape == (7, 101) and V.shape == (7, 100) and M.shape == (7, 100)
    assert st.shape == (7,) and st.dtype == torch.int32
    with pytest.raises(NotImplementedError):            # no CPU kernel behind the operator
        op(torch.zeros(3, dtype=torch.float64), torch.ones((), dtype=torch.float64), torch.ones(1, 2, dtype=torch.float64),
           torch.zeros(3, dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.float64), torch.zeros((), dtype=torch.float64))


def test_frame_dispatch_table_on_the_host():
    """r06: which kernel family and register-window width a frame of the reference's random range takes (FR:17-18: bays, stories ~ U{1..10}; half
    bandwidth 3 m + 2 along the short side m = min(stories, bays + 1)), the workspace the call asks for, and the plan signature a caller keeps its
    plan by -- all host-side functions of the library (no GPU call)."""
    from openpystruct_amd import _cabi
    lib = _cabi.load()
    B = 20000
    packed = 0
    for bays in range(1, 11):
        for stories in range(1, 11):
            m = min(stories, bays + 1)
            kd, n_eq = 3 * m + 2, 3 * stories * (bays + 1)
            sig = int(lib.ops_frame_plan_signature(B, n_eq, kd))
            fam, W, G, P = sig >> 24, (sig >> 16) & 0xFF, (sig >> 8) & 0xFF, sig & 0xFF
            if kd <= 29:
                packed += 1
                assert fam == 2 and W == (kd + 2) // 2 * 2 and P == (16 if kd <= 11 else 32) and G == (4 if (P == 16 or 23 < kd <= 27) else 2 if kd > 27 else 8), (bays, stories, sig)
                assert (kd // G + 1) * G + G <= P                      # the rows in flight below an entering group fit the lane group
                assert int(lib.ops_frame_workspace_bytes(B, n_eq, kd)) >= B * (n_eq + 3) * W * 8
            else:
                assert fam == 1 and W == 36 and P == 64, (bays, stories, sig)
                assert int(lib.ops_frame_workspace_bytes(B, n_eq, kd)) >= B * (n_eq + 4) * W * 8
    assert packed == 98                                               # 98 of the 100 draws (r06, late: kd 29 -- 9 x 9 .. -- joined)
    # beyond the tuned kernels: 56..63 the workgroup kernels (no plan), 64..1024 the column-by-column fallback, both with the band in the workspace
    assert lib.ops_frame_plan_signature(B, 2000, 59) == 0 and lib.ops_frame_plan_signature(B, 2000, 300) == 0
    assert lib.ops_frame_workspace_bytes(B, 2000, 300) >= B * 2000 * 301 * 8
    # small batches: no plan; the option moves the threshold (and is put back)
    assert lib.ops_frame_plan_signature(64, 90, 17) == 0
    try:
        assert lib.ops_amd_set_option(b"frame_latency_batch", 0) == _cabi.OK and lib.ops_frame_plan_signature(64, 90, 17) >> 24 == 2
        assert lib.ops_amd_set_option(b"frame_pack", 0) == _cabi.OK and lib.ops_frame_plan_signature(64, 90, 17) >> 24 == 1
    finally:
        lib.ops_amd_set_option(b"frame_latency_batch", -1); lib.ops_amd_set_option(b"frame_pack", 1)
    assert lib.ops_amd_get_option(b"deterministic") == 0


def _arg_buffer():
    """Pointer for the 'valid' arguments of the refusal checks below: 4 KiB of zeros on the GPU when one is visible, so that a C
    entry that stopped refusing and launched would still read and write memory this test owns (in bounds for every shape used)."""
    import numpy as np
    import torch
    if torch.cuda.is_available():
        t = torch.zeros(512, dtype=torch.float64, device="cuda")
        return t, t.data_ptr()
    a = np.zeros(512)
    return a, a.ctypes.data


def test_residual_vjp_entry_refuses_bad_arguments(lib):
    keep, p = _arg_buffer()
    B, Ne = 2, 3

    def call(B=B, Ne=Ne, null=None):
        ptrs = [None if k == null else p for k in range(13)]      # x, E, I, fix, v, theta, gv, gt, sv, st, dv, dt, dI
        x, E, I, fix, v, th, gv, gt, sv, st, dv, dt, dI = ptrs
        return lib.ops_beam_residual_vjp_f64(B, Ne, x, 0, E, 0, I, fix, 0, v, th, gv, gt, sv, st, dv, dt, dI, None)
    for k in range(13):
        assert call(null=k) == _cabi.ERR_INVALID_ARG, k
    assert call(Ne=0) == _cabi.ERR_INVALID_ARG and call(Ne=-1) == _cabi.ERR_INVALID_ARG and call(B=-1) == _cabi.ERR_INVALID_ARG
    assert call(B=0) == _cabi.OK and call(B=0, null=0) == _cabi.OK        # an empty batch is a no-op, checked before the pointers
    del keep


def test_deterministic_head_backward_refuses_a_null_ln_part(lib):
    """Deterministic mode: the head backward's LayerNorm sums go through per-workgroup partials; without a partial buffer the launch is
    refused before any HIP call (atomics would add the workgroups in arrival order)."""
    keep, p = _arg_buffer()
    a = _cabi.TfdHeadBwdArgs(B=4, S=2, d=16, hid=16, C=4, g=p, Wt2=p, Wt1=p, gamma=p, p_drop=0.0, a16=p, mean=p, rstd=p, h=p, d_a=p,
                             dcls_rows=p, dgamma=p, dbeta=p)
    try:
        assert lib.ops_amd_set_option(b"deterministic", 1) == _cabi.OK and lib.ops_amd_get_option(b"deterministic") == 1
        assert lib.ops_tfd_head_bwd(ctypes.byref(a), None) == _cabi.ERR_INVALID_ARG
    finally:
        lib.ops_amd_set_option(b"deterministic", 0)
    assert lib.ops_amd_get_option(b"deterministic") == 0
    del keep


def test_physics_loss_entries_refuse_bad_arguments(lib):
    keep, p = _arg_buffer()
    B, Ne = 2, 3
    N = Ne + 1
    assert lib.ops_physics_loss_part_doubles(B, Ne) == 8

    def args(rec=True, **kw):
        a = _cabi.PhysicsLossArgs(B=B, Ne=Ne, preds=p, preds_bf16=0, ldp=Ne if rec else Ne + 2 * N, I_scale=p, I_mean=p, I_min=1e-8,
                                  Fy=p, x=p, fix=p, E=2e11, wy=-1e3, weight=1.0, ev=p, et=p, part=p, value=p, dpreds=p)
        if rec:
            a.v_rec, a.t_rec = p, p
        else:
            a.v_scale, a.v_mean, a.t_scale, a.t_mean = p, p, p, p
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a):
        return (lib.ops_physics_loss_fwd(ctypes.byref(a), None) == _cabi.ERR_INVALID_ARG
                and lib.ops_physics_loss_bwd(ctypes.byref(a), None) == _cabi.ERR_INVALID_ARG)
    assert lib.ops_physics_loss_fwd(None, None) == _cabi.ERR_INVALID_ARG and lib.ops_physics_loss_bwd(None, None) == _cabi.ERR_INVALID_ARG
    for rec in (True, False):
        for name in ("preds", "I_scale", "I_mean", "Fy", "x", "fix", "ev", "et", "part"):
            assert refused(args(rec, **{name: None})), (rec, name)
        assert refused(args(rec, B=0)) and refused(args(rec, Ne=0)) and refused(args(rec, B=-1))
        assert refused(args(rec, ldp=Ne - 1 if rec else Ne + 2 * N - 1)), rec           # fewer columns than the term reads
        assert lib.ops_physics_loss_fwd(ctypes.byref(args(rec, value=None)), None) == _cabi.ERR_INVALID_ARG      # its output missing
        assert lib.ops_physics_loss_bwd(ctypes.byref(args(rec, dpreds=None)), None) == _cabi.ERR_INVALID_ARG
    assert refused(args(True, t_rec=None)) and refused(args(True, v_rec=None))     # one recorded field without the other
    for name in ("v_scale", "v_mean", "t_scale", "t_mean"):                        # predicted fields without their scalers
        assert refused(args(False, **{name: None})), name
    del keep
