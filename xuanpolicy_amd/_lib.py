"""ctypes binding of the C ABI in include/xuanpolicy_amd.h (libxuanpolicy_amd.so, gfx950).

The library is built in-tree by `build_library()` (hipcc, --offload-arch=gfx950) and loaded after
`import torch`, so its NEEDED libamdhip64.so.7 resolves to the HIP runtime torch already mapped
(same SONAME) and torch's device pointers and hipStream_t handles are valid in it.

There is no CPU fallback: every entry point raises if the library is missing or a call fails.
"""
import ctypes
import os
import re
import subprocess

import torch  # noqa: F401  (must be loaded first: see module docstring)

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "libxuanpolicy_amd.so")
CSRC = os.path.join(PKG_DIR, "csrc")
SOURCES = ["gae.hip", "loss.hip", "rollout.hip", "optim.hip", "mlp.hip", "head.hip", "thin.hip", "per.hip", "atari.hip",
           "classic.hip", "dqn.hip", "conv.hip", "igemm.hip", "smallmlp.hip", "sgemm3.hip"]
HEADER = os.path.join(REPO_DIR, "include", "xuanpolicy_amd.h")


class XpaError(RuntimeError):
    pass


# The type spellings include/xuanpolicy_amd.h may use for scalars; any declarator with a `*` is a c_void_p.
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "unsigned": ctypes.c_uint, "uint8_t": ctypes.c_uint8, "float": ctypes.c_float, "double": ctypes.c_double,
            "xpa_stream_t": ctypes.c_void_p}


def _ctype(type_name, declarator, where):
    """ctypes type of `type_name declarator` (declarator: `name`, `*name`, `**name`); raises rather than guess."""
    name = declarator.replace("*", " ").strip()
    if not name.isidentifier() or ("*" not in declarator and type_name not in _SCALARS):
        raise XpaError("cannot bind '%s %s' in %s" % (type_name, declarator, where))
    return name, (ctypes.c_void_p if "*" in declarator else _SCALARS[type_name])


def parse_header(text):
    """Parse a C header in the subset include/xuanpolicy_amd.h is written in.

    Returns (signatures, structs, constants): name -> (restype, argtypes) for every `ret xpa_name(args);`, a
    ctypes.Structure subclass for every `typedef struct Name { ... } Name;` and the integer `#define XPA_*`s."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(XPA_\w+)[ \t]+(\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$|\bconst\b", " ", text, flags=re.M)   # const does not change a binding
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", text):
        fields = []
        for line in filter(None, (ln.strip() for ln in body.split(";"))):
            m = re.fullmatch(r"(\w+)\s+(.+)", line, re.S)
            if not m:
                raise XpaError("cannot bind '%s' in struct %s" % (line, name))
            fields += [_ctype(m[1], d.strip(), "struct " + name) for d in m[2].split(",")]
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
    signatures = {}
    for ret, name, args in re.findall(r"(\w+)\s+(xpa_\w+)\s*\(([^()]*)\)\s*;", text):
        if ret != "void" and ret not in _SCALARS:
            raise XpaError("cannot bind return type '%s' of %s" % (ret, name))
        argtypes = []
        for arg in ([] if args.strip() == "void" else args.split(",")):
            m = re.fullmatch(r"\s*(\w+)\s+([*\s]*\w+)\s*", arg)
            if not m:
                raise XpaError("cannot bind '%s' in %s" % (" ".join(arg.split()), name))
            argtypes.append(_ctype(m[1], m[2], name)[1])
        signatures[name] = (None if ret == "void" else _SCALARS[ret], argtypes)
    missed = set(re.findall(r"\b(xpa_\w+)\s*\(", text)) - set(signatures)
    if missed:
        raise XpaError("cannot parse the declaration of %s" % ", ".join(sorted(missed)))
    return signatures, structs, constants


# The header is the only statement of the ABI: name -> (restype, argtypes), the argument structs and the constants.
with open(HEADER) as _f:
    SIGNATURES, _structs, _constants = parse_header(_f.read())
XpaSmallMlpArgs, XpaSmallRolloutArgs = _structs["XpaSmallMlpArgs"], _structs["XpaSmallRolloutArgs"]
XpaSmallRolloutHead, XpaSmallMlpGauss = _structs["XpaSmallRolloutHead"], _structs["XpaSmallMlpGauss"]
XpaSmallCloseArgs, XpaSmallEval = _structs["XpaSmallCloseArgs"], _structs["XpaSmallEval"]
ABI_VERSION, COLSUM_TICKET_INTS = _constants["XPA_ABI_VERSION"], _constants["XPA_COLSUM_TICKET_INTS"]
ENV_CODES = {n: v for n, v in _constants.items() if n.startswith("XPA_ENV_")}   # xpa_small_rollout_batch's `env`

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall"]
OBJ_DIR = os.path.join(PKG_DIR, "_obj")

_lib = None


def _digest(paths, extra=""):
    import hashlib
    h = hashlib.sha256(extra.encode())
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build_library(force=False, verbose=False, jobs=None):
    """Compile csrc/*.hip into libxuanpolicy_amd.so for gfx950 (cross-compiles without a GPU).

    One hipcc process per source file (in parallel, objects under xuanpolicy_amd/_obj/), then one link step.
    An object is rebuilt when the content hash of its source + the shared headers + the flags differs from the
    one recorded beside it (mtimes raced: a source edited while a build was running kept a stale object that
    looked newer than it)."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    headers = sorted([os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")] + [HEADER])
    hdr_digest = _digest(headers, " ".join(HIPCC_FLAGS))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ_DIR, exist_ok=True)
    rebuilt = []

    def compile_one(src):
        obj = os.path.join(OBJ_DIR, os.path.basename(src) + ".o")
        want = _digest([src], hdr_digest)
        stamp = obj + ".sha256"
        if not force and os.path.exists(obj) and os.path.exists(stamp):
            with open(stamp) as f:
                if f.read().strip() == want:
                    return obj
        cmd = [hipcc] + HIPCC_FLAGS + ["-c", "-o", obj + ".tmp", src]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(obj + ".tmp", obj)
        with open(stamp, "w") as f:
            f.write(want)
        rebuilt.append(obj)
        return obj
    jobs = jobs or min(len(srcs), max(1, min(16, os.cpu_count() or 1)))
    with ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(compile_one, srcs))
    link_stamp = LIB_PATH + ".sha256"
    link_want = _digest(objs)
    if not force and not rebuilt and os.path.exists(LIB_PATH) and os.path.exists(link_stamp):
        with open(link_stamp) as f:
            if f.read().strip() == link_want:
                return LIB_PATH
    tmp = LIB_PATH + ".tmp"
    cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", tmp] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(tmp, LIB_PATH)
    with open(link_stamp, "w") as f:
        f.write(link_want)
    return LIB_PATH


def load(path=None):
    """Load the library (once) and bind every exported symbol's signature."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise XpaError("libxuanpolicy_amd.so not built (%s); run __graft_entry__.build() or "
                       "xuanpolicy_amd._lib.build_library()" % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.xpa_abi_version()
    if v != ABI_VERSION:
        raise XpaError("ABI version mismatch: library %d, bindings %d" % (v, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise XpaError("%s failed: hipError %d%s" % (what, rc, " (invalid argument)" if rc == 1 else ""))


def call(fn, *args):
    """Call a status-returning entry point; a non-zero status raises, named after the symbol that ran."""
    check(fn(*args), fn.__name__)
