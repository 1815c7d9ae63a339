"""ctypes binding of libcvk.so, derived from include/cvk.h (see _header.py).  There is NO fallback: if the HIP library is missing or
cannot be loaded the product path raises — a silent eager/CPU path would void every parity claim."""
import ctypes
import os
import subprocess
import threading

from . import _header
from ._header import CvkError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CVK_LIB_PATH") or os.path.join(_HERE, "lib", "libcvk.so")   # override: kernel experiments only
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "cvk.h")

_H = _header.read(HEADER)               # once, at import: engine.py needs View then
SIGNATURES = _H.prototypes              # name -> (restype, argtypes); device pointers are c_void_p and are passed as integers

# header name -> name in this module
_NAMES = {
    "cvk_view": "View", "cvk_viewh": "ViewH", "cvk_augment_record": "AugmentRecord", "cvk_crop_record": "CropRecord",
    "cvk_adamw_hyper": "AdamwHyper", "cvk_sgd_hyper": "SgdHyper", "cvk_adamw_range": "AdamwRange", "cvk_norm_segment": "NormSegment",
    "cvk_pack_job": "PackJob", "cvk_colsum_job": "ColsumJob", "cvk_wt_job": "WtJob", "cvk_wreduce_job": "WReduceJob",
    "CVK_STAT_ROWS": "CVK_STAT_ROWS", "CVK_ADAMW_ARG_RECORDS": "ADAMW_ARG_RECORDS",
    "CVK_PACK_BATCH_MAX": "PACK_BATCH_MAX", "CVK_COLSUM_BATCH_MAX": "COLSUM_BATCH_MAX", "CVK_WREDUCE_BATCH_MAX": "WREDUCE_BATCH_MAX",
    "CVK_WT_BATCH_MAX": "WT_BATCH_MAX",
}
globals().update({py: (_H.structs if c in _H.structs else _H.defines)[c] for c, py in _NAMES.items()})
DEFINES = _H.defines                    # every integer #define of the header, under its header name

STEP_LOG_COLUMNS = 5                    # cvk_step_log row without a clip record: loss, lr, beta1, ||gw||_2, ||gb||_2
STEP_LOG_NORM_COLUMNS = 7               # cvk_step_log row with one: the five, then total_norm and clip_coef of the step

_lib = None
_lock = threading.Lock()


def build(verbose=False):
    """Compile csrc/*.hip and csrc/side.cpp (host code) for gfx950 into lib/libcvk.so (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode != 0:
        raise CvkError("building libcvk.so failed (hipcc --offload-arch=gfx950); see output above")
    return LIB_PATH


def header_abi_hash(path=None):
    """First 64 bits of the SHA-256 of include/cvk.h — what csrc/Makefile stamps into the library as CVK_ABI_HASH."""
    import hashlib
    with open(path or HEADER, "rb") as f:
        return int(hashlib.sha256(f.read()).hexdigest()[:16], 16)


def check_abi(lib, header=None):
    """Refuse a library compiled against another include/cvk.h than the one the binding is derived from: entry points keep
    their names when argument lists change and ctypes does not check arity, so a stale libcvk.so would corrupt calls silently."""
    try:
        fn = lib.cvk_abi_hash
    except AttributeError:
        raise CvkError(f"{LIB_PATH} exports no cvk_abi_hash: it predates the ABI stamp; rebuild it (make -C {CSRC})") from None
    fn.restype, fn.argtypes = SIGNATURES["cvk_abi_hash"]
    got, want = fn(), header_abi_hash(header)
    if got != want:
        raise CvkError(f"{LIB_PATH} was built from another include/cvk.h (library stamp {got:016x}, header {want:016x}); "
                       f"rebuild it: make -C {CSRC}")


def bind(cdll, names=None):
    """Set restype and argtypes on a ctypes.CDLL of the library, for every entry point of the header or (an older build that lacks
    some: the tools' baselines) for `names` only; returns the handle."""
    for name in SIGNATURES if names is None else names:
        fn = getattr(cdll, name)  # AttributeError here = ABI drift between header and library
        fn.restype, fn.argtypes = SIGNATURES[name]
    return cdll


def load():
    """Load libcvk.so once.  Raises CvkError when it is missing — there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  torch's bundled libamdhip64 (SONAME libamdhip64.so.7) must be the one HIP runtime in-process
        if not os.path.exists(LIB_PATH):
            raise CvkError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950).  pytorch_camvid_amd has no CPU/eager fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        check_abi(lib)
        bind(lib)
        if lib.cvk_version() != DEFINES["CVK_VERSION"]:
            raise CvkError(f"libcvk.so version {lib.cvk_version()} != CVK_VERSION {DEFINES['CVK_VERSION']} of include/cvk.h")
        _lib = lib
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = load().cvk_last_error_string()
        raise CvkError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
