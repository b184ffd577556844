"""The launch epilogue and the lists that are stated once, without a GPU: what the tree's own sources say, and
opsamd::launch_status / launch_refused themselves in a stand-alone host program (tests/csrc/launch_status_main.cpp, linked with
csrc/library.hip; HIP's error strings need no device)."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpystruct_amd", "csrc")
LIBRARY = ("library.hpp", "library.hip")

SOURCES = ["beam_solve.hip", "beam_fat.hip", "sizing_step.hip", "beam_residual.hip", "frame_solve.hip", "stencil_bn.hip", "flat_adam.hip",
           "fused_loss.hip", "fused_bn.hip", "input_prep.hip", "mlp_block.hip", "seq_block.hip", "seq_layer.hip", "mem_bench.hip",
           "case_draw.hip", "bayes_mlp.hip", "beam_vjp.hip", "frame_vjp.hip", "sizing_grad.hip", "frame_sizing_grad.hip", "frame_loads.hip",
           "sizing_multicase.hip", "frame_designs.hip", "design_loss.hip", "frame_groups.hip", "library.hip"]
EXTENSION_HEADERS = ["openpystruct_amd_frame_vjp.h", "openpystruct_amd_frame_sizing.h", "openpystruct_amd_frame_loads.h",
                     "openpystruct_amd_sizing_multicase.h", "openpystruct_amd_frame_cases.h", "openpystruct_amd_frame_designs.h",
                     "openpystruct_amd_design_loss.h", "openpystruct_amd_frame_groups.h", "openpystruct_amd_sizing_grad.h"]


def _texts():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(paths) > 40
    return {os.path.basename(p): open(p).read() for p in paths}


def _entry_bodies(text):
    """(name, body) of every `extern "C" int ops_...` definition of a source text."""
    for m in re.finditer(r'extern "C" int (ops_\w+)\(', text):
        close = text.index(")", m.end())                  # (no entry takes a function pointer: its arguments hold no parentheses)
        assert "(" not in text[m.end():close], m.group(1)
        if text[close + 1:].lstrip()[:1] != "{":
            continue                                      # a declaration
        start = text.index("{", close)
        depth, i = 1, start + 1
        while depth:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        yield m.group(1), text[start:i]


def test_the_launch_code_and_its_message_are_returned_in_one_place():
    texts = _texts()
    for name, text in texts.items():
        if name not in LIBRARY:
            assert "OPS_AMD_ERR_LAUNCH" not in text, name
            assert "hipGetErrorString" not in text, name
        assert "== hipSuccess ? OPS_AMD_OK" not in text, name
    assert "OPS_AMD_ERR_LAUNCH" in texts["library.hpp"] and "hipGetErrorString" in texts["library.hpp"]
    launching = 0
    for name, text in texts.items():
        bodies = [body for _, body in _entry_bodies(text)]
        if any("hipLaunchKernelGGL" in body for body in bodies):
            launching += 1
            assert "launch_status(" in text, name
    assert launching >= 10      # (the scan finds the entries: it does not pass by finding none)


def test_the_sizing_step_launch_is_stated_once():
    texts = _texts()
    for name, text in texts.items():
        assert "{I, I64, nullptr, exp_avg" not in text, name
        if name != "sizing_math.hpp":
            assert "(G + 3) / 4" not in text and "(B + 3) / 4" not in text, name
    for name in ("sizing_step.hip", "sizing_grad.hip", "sizing_multicase.hip", "frame_designs.hip", "frame_groups.hip"):
        assert "launch_wave_rows(" in texts[name] and "kSizingMaxElems" in texts[name] + texts["frame_designs_math.hpp"], name
    for name in ("sizing_step.hip", "sizing_grad.hip", "sizing_multicase.hip", "beam_solve.hip", "frame_designs_math.hpp"):
        assert "sizing_args(" in texts[name], name


def test_the_build_and_the_binding_keep_no_second_list():
    from openpystruct_amd import _cabi, build
    assert not hasattr(build, "HEADERS")
    assert len(build.SOURCES) == 26 and len(_cabi.EXTENSION_HEADER_PATHS) == 9
    assert list(build.SOURCES) == [os.path.join(CSRC, f) for f in SOURCES]
    assert list(_cabi.EXTENSION_HEADER_PATHS) == [os.path.join(ROOT, "include", f) for f in EXTENSION_HEADERS]
    watched = {os.path.relpath(p, ROOT) for s in build.SOURCES for p in build._deps(s)}
    assert os.path.join("openpystruct_amd", "csrc", "library.hpp") in watched
    assert {os.path.join("include", f) for f in EXTENSION_HEADERS} <= watched


def test_the_stand_alone_experiment_build_needs_no_library_hip(tmp_path):
    """csrc/mlp_block.hip under MB_EXP is built alone (the recipe at the head of scripts/mlp_launch_bench.py) with its own stub of
    set_last_error.  Host side only, linked with undefined symbols refused: the one symbol that may be missing is the device code
    this compile leaves out."""
    from openpystruct_amd import build
    r = subprocess.run([build.hipcc_path(), f"--offload-arch={build.ARCH}", "--offload-host-only", "-O1", "-std=c++17", "-fPIC", "-shared",
                        "-DMB_EXP=1", "-Wl,-z,defs", "-o", str(tmp_path / "libmlp_exp1_host.so"), os.path.join(CSRC, "mlp_block.hip")],
                       capture_output=True, text=True, timeout=300)
    undefined = re.findall(r"undefined symbol: (.+)", r.stderr)
    assert undefined or r.returncode == 0, r.stderr
    assert [s for s in undefined if not s.startswith("__hip_fatbin")] == [], r.stderr


def test_launch_status_on_the_host(tmp_path):
    from openpystruct_amd import build
    prog = str(tmp_path / "launch_status_main")
    subprocess.check_call([build.hipcc_path(), f"--offload-arch={build.ARCH}", "-std=c++17", "-O1", "-Wall", "-pthread", "-x", "hip", "-o", prog,
                           os.path.join(ROOT, "tests", "csrc", "launch_status_main.cpp"), os.path.join(CSRC, "library.hip")])
    r = subprocess.run([prog], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
