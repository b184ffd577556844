"""ctypes binding of the C ABI, read from include/openpystruct_amd.h: the header is the one place where the entry points, their
argument structs and the OPS_* constants are written down; nothing here repeats a field, an argument list or a value.  Entry points
added without touching that header's declarations come from extension headers next to it (EXTENSION_HEADER_PATHS), read the same way.

The product path has NO CPU fallback: if the HIP shared library is missing or cannot be
loaded this module raises, loudly, instead of computing anything elsewhere.
"""
from __future__ import annotations

import ctypes
import os
import re
import types

_PKG = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_PKG), "include")
HEADER_PATH = os.path.join(_INCLUDE, "openpystruct_amd.h")
# additions to the C ABI that change no declaration of HEADER_PATH (and so not OPS_AMD_ABI_VERSION) have headers of their own, read in
# this order: a header may name the structs of the headers before it
EXTENSION_HEADER_PATHS = tuple(os.path.join(_INCLUDE, f"openpystruct_amd_{name}.h") for name in (
    "frame_vjp", "frame_sizing", "frame_loads", "sizing_multicase", "frame_cases", "frame_designs", "design_loss", "frame_groups", "sizing_grad"))
# extension headers added after the list above was pinned by name and length (tests/test_launch_status.py): read after it, the same way
LATER_EXTENSION_HEADER_PATHS = tuple(os.path.join(_INCLUDE, f"openpystruct_amd_{name}.h") for name in ("frame_frequency",))
# OPS_AMD_LIB lets A/B kernel experiments point at another build of the same C ABI
LIB_PATH = os.environ.get("OPS_AMD_LIB") or os.path.join(_PKG, "lib", "libopenpystruct_amd.so")


class ExtensionMissingError(RuntimeError):
    pass


# Every type word the header may use.  By value: the ctypes type of the same name and width (None: only behind a pointer).
# Pointers: `char*` is c_char_p, a pointer to a struct of the header POINTER(that Structure), every other pointer at any depth
# c_void_p -- the one argtype that takes what the callers pass: tensor.data_ptr() integers, None, ctypes.byref(...) and ctypes arrays.
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "long": ctypes.c_long,
            "long long": ctypes.c_longlong, "unsigned": ctypes.c_uint, "unsigned long long": ctypes.c_ulonglong,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
            "void": None, "char": None, "uint8_t": None}
_DECLARATION = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;"        # typedef struct NAME { fields } NAME;
                          r"|([\w\s*]+?)\b(ops_\w+)\s*\(([^()]*)\)\s*;)")                      # RET ops_xxx(ARGS);
_INTEGER = re.compile(r"(0[xX][0-9a-fA-F]+|[0-9]+)[uU]?")


def _ctype(base: str, depth: int, structs: dict, where: str):
    """ctypes type of `depth` pointers to the type named by the words `base`."""
    if base not in _SCALARS and base not in structs:
        raise ValueError(f"{where}: unknown type {base!r}")
    if depth == 0:
        if _SCALARS.get(base) is None:
            raise ValueError(f"{where}: {base!r} by value")
        return _SCALARS[base]
    if depth == 1 and base == "char":
        return ctypes.c_char_p
    return ctypes.POINTER(structs[base]) if depth == 1 and base in structs else ctypes.c_void_p


def _declarators(text: str, structs: dict, where: str, named: bool = True) -> list:
    """(name, ctypes type) of every declarator of `TYPE [*]a, [*]b`; named=False: a bare type (the return type of a prototype)."""
    out, base = [], None
    for piece in text.split(","):
        words = piece.replace("*", " ").split()
        if not all(map(str.isidentifier, words)):       # an array, a bit field, a function pointer, an initialiser
            raise ValueError(f"{where}: cannot read {text.strip()!r}")
        words = [w for w in words if w != "const"]
        name = words.pop() if named and words else None
        if named and (name is None or name in _SCALARS or name in structs):
            raise ValueError(f"{where}: no name in {text.strip()!r}")
        if base is None:
            base = " ".join(words)
        elif words:                                     # the later declarators of a line are stars and a name
            raise ValueError(f"{where}: cannot read {text.strip()!r}")
        out.append((name, _ctype(base, piece.count("*"), structs, where)))
    return out


def read_header(text: str, known_structs: dict = None) -> types.SimpleNamespace:
    """Parse the text of a C header of the shape of include/openpystruct_amd.h into
         defines    {OPS_NAME: int}                        every `#define OPS_... <integer literal>`
         structs    {c_name: ctypes.Structure subclass}    every `typedef struct NAME { ... } NAME;`
         functions  {c_name: (restype, [argtypes])}        every prototype `RET ops_xxx(ARGS);`
    Comments, the other preprocessor lines and the `extern "C"` braces are dropped; every character that remains must belong to one
    of the two declaration forms and every type word must be known, else ValueError with the offending text -- nothing is skipped.
    `known_structs`: structs of a header this one includes (an extension header's argument lists may name them); they may be used, not
    declared again, and are not part of the result."""
    out = types.SimpleNamespace(defines={}, structs={}, functions={})
    scope = dict(known_structs or {})
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    if "\\\n" in text:
        raise ValueError("line continuation in the header")
    code = []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.match(r"\s*#\s*define\s+(OPS_\w+)(.*)", line)
        if m:
            if not _INTEGER.fullmatch(m.group(2).strip()):
                raise ValueError(f"#define {m.group(1)}: not an integer literal: {m.group(2).strip()!r}")
            out.defines[m.group(1)] = int(m.group(2).strip().rstrip("uU"), 0)
    text = "\n".join(code)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, flags=re.S)
    text = (m.group(1) if m else text).rstrip()
    pos = 0
    while pos < len(text):
        m = _DECLARATION.match(text, pos)
        if not m:
            raise ValueError(f"cannot read the header at: {text[pos:pos + 120].strip()!r}")
        pos = m.end()
        tag, body, name, ret, func, args = m.groups()
        if func is None:
            if tag != name or name in scope:
                raise ValueError(f"struct {tag}: typedef'd as {name}" if tag != name else f"struct {name} declared twice")
            fields = [f for decl in body.split(";") if decl.strip() for f in _declarators(decl, scope, f"struct {name}")]
            camel = "".join(w.capitalize() for w in name[4 * name.startswith("ops_"):].split("_"))      # ops_tfd_head_bwd_args -> TfdHeadBwdArgs
            out.structs[name] = scope[name] = type(camel, (ctypes.Structure,), {"_fields_": fields})
        else:
            if func in out.functions:
                raise ValueError(f"{func} declared twice")
            params = [] if args.strip() == "void" else [_declarators(a, scope, func)[0][1] for a in args.split(",")]
            restype = None if ret.split() == ["void"] else _declarators(ret, scope, func, named=False)[0][1]
            out.functions[func] = (restype, params)
    return out


def _read_abi(path: str = "", known_structs: dict = None) -> types.SimpleNamespace:
    path = path or HEADER_PATH
    try:
        with open(path) as f:
            return read_header(f.read(), known_structs)
    except OSError as e:
        raise ExtensionMissingError(f"{path} not readable ({e}): the ctypes binding is derived from the C header") from e


_abi = _read_abi()
EXPORTS = tuple(_abi.functions)     # every symbol include/openpystruct_amd.h declares
# prototypes and the argument structs that are new with them (they may name the structs of the main header and of the extension
# headers listed before them, not redeclare them)
_extensions, _known_structs = {}, dict(_abi.structs)
for _path in EXTENSION_HEADER_PATHS + LATER_EXTENSION_HEADER_PATHS:
    _extensions[_path] = _read_abi(_path, _known_structs)
    _known_structs.update(_extensions[_path].structs)
for _path, _ext in _extensions.items():
    if _ext.defines or set(_ext.functions) & set(EXPORTS):
        raise ValueError(f"{_path}: an extension header declares new entry points and their argument structs, nothing else")
EXTENSION_EXPORTS = tuple(name for _ext in _extensions.values() for name in _ext.functions)
_struct = _abi.structs.__getitem__
SizingParams = _struct("ops_sizing_params")
PhysicsLossArgs = _struct("ops_physics_loss_args")
MlpStripArgs = _struct("ops_mlp_strip_args")
MlpWgradProblem = _struct("ops_mlp_wgrad_problem")
MlpRepackEntry = _struct("ops_mlp_repack_entry")
WgradProblem = _struct("ops_wgrad_problem")
TfdLayerArgs = _struct("ops_tfd_layer_args")
TfdLayerBwdArgs = _struct("ops_tfd_layer_bwd_args")
TfdHeadArgs = _struct("ops_tfd_head_args")
TfdHeadBwdArgs = _struct("ops_tfd_head_bwd_args")
TfdFrontArgs = _struct("ops_tfd_front_args")
TfdFrontBwdArgs = _struct("ops_tfd_front_bwd_args")
BayesLayer = _struct("ops_bayes_layer")
BayesMcArgs = _struct("ops_bayes_mc_args")
_extension_structs = {name: cls for _ext in _extensions.values() for name, cls in _ext.structs.items()}
SizingObjective = _extension_structs["ops_sizing_objective"]
FrameSizingObjective = _extension_structs["ops_frame_sizing_objective"]
DesignLossArgs = _extension_structs["ops_design_loss_args"]
# every OPS_AMD_X / OPS_X of the header as X: OK, ERR_*, FIX_*, ABI_VERSION, FRAME_REUSE_PLAN, MLP_*, BAYES_*, WGRAD_MAX_GROUP, ADAM_*, ...
for _name, _value in _abi.defines.items():
    _short = _name[len("OPS_AMD_"):] if _name.startswith("OPS_AMD_") else _name[len("OPS_"):]
    if _short in globals():
        raise ValueError(f"{HEADER_PATH}: {_name} collides with _cabi.{_short}")
    globals()[_short] = _value

_lib = None


def load():
    """Load the HIP library once; raise ExtensionMissingError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ExtensionMissingError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m openpystruct_amd.build` "
            "(needs hipcc). openpystruct_amd has no CPU fallback for the beam solve."
        )
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise ExtensionMissingError(f"cannot load {LIB_PATH}: {e}") from e
    declared = [(HEADER_PATH, _abi)] + list(_extensions.items())
    for header, name, restype, argtypes in [(h, n, *sig) for h, abi in declared for n, sig in abi.functions.items()]:
        try:
            f = getattr(lib, name)
        except AttributeError as e:
            raise ExtensionMissingError(f"{LIB_PATH} does not export {name}, which {header} declares: rebuild with "
                                        "`python -m openpystruct_amd.build --force`") from e
        f.restype, f.argtypes = restype, argtypes
    if lib.ops_amd_abi_version() != ABI_VERSION:     # a stale build of another ABI must not be driven with today's argument lists
        raise ExtensionMissingError(f"{LIB_PATH} has C-ABI version {lib.ops_amd_abi_version()}, "
                                    f"this package needs {ABI_VERSION}: rebuild with `python -m openpystruct_amd.build --force`")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    """Raise for the return code of a launch function that is not OK, with the library's message for this thread when there is one."""
    if rc != OK:
        msg = load().ops_amd_last_error().decode()
        raise RuntimeError(f"{what} failed with code {rc}" + (f": {msg}" if msg else ""))


def set_option(name: str, value: int) -> None:
    """include/openpystruct_amd.h ops_amd_set_option: "frame_latency_batch" (-1 = the library's model, 0 = tuned kernels for every batch),
    "frame_pack" (0 = one wave per frame for every half bandwidth), "frame_coop" (0 / 1 / 2: four waves per frame for small batches never / where
    measured faster / always), "deterministic".  The library reads no environment variable."""
    if load().ops_amd_set_option(name.encode(), int(value)) != OK:
        raise ValueError(f"unknown library option {name!r}")


def get_option(name: str) -> int:
    v = int(load().ops_amd_get_option(name.encode()))
    if v == -2:
        raise ValueError(f"unknown library option {name!r}")
    return v
