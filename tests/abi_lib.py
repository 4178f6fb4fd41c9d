"""The one parser of include/seir_hip.h behind the binding tests: every `seir_*` prototype with its return type and its
parameter list, the one map from the header's C types to ctypes, and the check that a product's test makes of the symbols it
pins -- declared with exactly these parameters, exported, bound with the header's types.  tests/test_abi.py runs the
types of every prototype, pinned or not."""
import ctypes
import os
import re

import __graft_entry__ as entry
from covid19uk_amd import _lib

HEADER = os.path.join(entry.ROOT, "include", "seir_hip.h")
# a handle is an opaque pointer to the binding; a struct pointer is a pointer to the binding's mirror of the struct
CTYPE = {
    "int": ctypes.c_int, "void": None, "void *": ctypes.c_void_p, "const char *": ctypes.c_char_p,     # the return types
    "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double,
    "seir_ctx *": ctypes.c_void_p, "const seir_ctx *": ctypes.c_void_p, "seir_sampler *": ctypes.c_void_p,
    "seir_ctx **": ctypes.POINTER(ctypes.c_void_p), "seir_sampler **": ctypes.POINTER(ctypes.c_void_p),
    "void **": ctypes.POINTER(ctypes.c_void_p), "const void *": ctypes.c_void_p,
    "const seir_desc *": ctypes.POINTER(_lib.SeirDesc), "const seir_sampler_desc *": ctypes.POINTER(_lib.SeirSamplerDesc),
    "const seir_sim_desc *": ctypes.POINTER(_lib.SeirSimDesc), "seir_sweep_plan *": ctypes.POINTER(_lib.SeirSweepPlan),
    "seir_product_state *": ctypes.POINTER(_lib.SeirProductState),
}
for _c, _t in (("float", ctypes.c_float), ("double", ctypes.c_double), ("int32_t", ctypes.c_int32), ("int64_t", ctypes.c_int64),
               ("uint32_t", ctypes.c_uint32), ("uint64_t", ctypes.c_uint64)):
    CTYPE[_c + " *"] = CTYPE["const " + _c + " *"] = ctypes.POINTER(_t)


def prototypes():
    """{name: (return type, [parameter, ...])} of every `seir_*` prototype, comments stripped and blanks normalised:
    `"seir_sampler_load_status": ("int", ["seir_sampler *s", "uint64_t out[8]", "int32_t clear"])`; `(void)` is `[]`."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^((?:const )?\w+ \*?)(seir_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = " ".join(params.split())
        out[name] = (ret.strip(), [] if params == "void" else [p.strip() for p in params.split(",")])
    return out


def c_type(p):
    """A parameter's C type as CTYPE spells it: `const int64_t *ranks` -> `const int64_t *`, `seir_ctx **out` -> `seir_ctx **`,
    `uint64_t out[8]` -> `uint64_t *` (an array parameter is a pointer)."""
    ty = p.strip().rsplit(" ", 1)[0] + (" *" if "*" in p or "[" in p else "")
    return ty + "*" if "**" in p else ty


def check_symbols(new):
    """`new` {name: parameter list}: each is declared in the header with exactly that parameter list, names included,
    exported, and bound with the header's types -- no void pointer in place of a typed one.  Returns the loaded library."""
    entry.build()
    lib = _lib.load()
    declared = prototypes()
    for name, params in new.items():
        assert name in declared, f"{name} is not declared in include/seir_hip.h"
        ret, plist = declared[name]
        assert ", ".join(plist) == params, (name, ", ".join(plist))
        assert name in _lib.exported_symbols()
        fn = getattr(lib, name)                              # exported by the library
        want = [CTYPE[c_type(p)] for p in plist]
        assert fn.restype is CTYPE[ret] and list(fn.argtypes) == want, (name, fn.restype, fn.argtypes)
    return lib
