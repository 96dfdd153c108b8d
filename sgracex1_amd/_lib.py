"""ctypes binding of libsgx.so, derived at import from include/sgx.h (the only declaration of the C ABI).

_abi.py reads the header; this module loads the library and publishes what the header declares under the names the
rest of the package uses: every #define and enumerator as `SGX_*`, every struct as the CamelCase of its C name without
`sgx_` (`sgx_layer_desc` -> `LayerDesc`), the function names as `SYMBOLS`, and `lib` with argtypes / restype set on
each of them.  A new entry point, field or constant is declared in sgx.h and nowhere else.

The library is the only backend.  If it is missing or does not load, importing this module
raises -- there is no CPU or PyTorch fallback for the accelerated path.
"""
import contextlib
import ctypes
import os

# PyTorch-ROCm ships its own HIP runtime; importing it first makes that copy the one this process
# (and libsgx.so, whose libamdhip64 dependency then resolves to it) uses -- two runtimes in one
# process cannot share streams or allocations.
import torch  # noqa: F401

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# SGX_LIB_PATH selects another build of the same library (tools/sweep_spmm.py compares variants); the header is the same
LIB_PATH = os.environ.get("SGX_LIB_PATH") or os.path.join(_HERE, "csrc", "libsgx.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sgx.h")      # the file build.py compiles against

with open(HEADER_PATH) as _f:
    ABI = _abi.read_header(_f.read(), HEADER_PATH)
globals().update(ABI.constants)
globals().update({cls.__name__: cls for cls in ABI.structs.values()})
SYMBOLS = list(ABI.functions)


class SgxError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        super().__init__(f"{where}: {status_string(status)} (sgx_status {status})")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP library first (python -m sgracex1_amd.build); "
            "sgracex1_amd has no other backend")
    lib = ctypes.CDLL(LIB_PATH)
    _abi.bind(lib, ABI)
    return lib


lib = _load()


def status_string(status):
    return lib.sgx_status_string(int(status)).decode()


def check(status, where):
    if status != 0:
        raise SgxError(status, where)


@contextlib.contextmanager
def tuning(**overrides):
    """Run a block under SGX_* tuning overrides: `with tuning(SGX_XW_NO_WLDS="1"): ...`.  The library reads its
    overrides from the environment once per process (include/sgx.h, sgx_reload_env), so changing os.environ alone does
    nothing after the first call; this sets the variables, has the library read them again, and undoes both on the way
    out.  A value of None removes the variable for the block.  For tests and probes that compare two forms of a kernel."""
    saved = {k: os.environ.get(k) for k in overrides}
    try:
        for k, v in overrides.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        lib.sgx_reload_env()
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.sgx_reload_env()
