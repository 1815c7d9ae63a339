"""CPU-side checks of the C-ABI boundary: libcvk.so loads, exports exactly what include/cvk.h declares, and the
Python binding table, which _header.py derives from that header, matches.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "cvk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cvk_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_expected_surface():
    syms = header_symbols()
    assert "cvk_conv3x3_fwd" in syms and "cvk_conv3x3_wgrad" in syms and "cvk_softmax_ce_fwd" in syms
    assert len(syms) >= 30


def test_library_builds_loads_and_exports_every_declared_symbol():
    from pytorch_camvid_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.cvk_version() == 100
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in header_symbols():
        assert hasattr(raw, s), f"{s} declared in include/cvk.h but not exported by libcvk.so"
    assert sorted(_lib.SIGNATURES) == header_symbols(), "Python binding table out of sync with include/cvk.h"


SNIPPET = """
/* a comment with cvk_fake(int); in it, and (parentheses; semicolons) */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define CVK_A 7             /* plain */
#define CVK_B (-3)          // parenthesised and negative; cvk_fake2(int);
#define CVK_C -4
#define CVK_D (12)
#define CVK_E 0x10
#define CVK_TEXT "no"
#define CVK_EXPR (1 << 3)
typedef struct cvk_v { float* ptr; int64_t sN, sY, sX; } cvk_v;
typedef struct cvk_rec {
    unsigned long long n;      /* cvk_fake3(int); */
    uint8_t x[256];
    int rows, cols[3], tile;
    const void* p;
    cvk_v inner;
} cvk_rec;
int cvk_three_lines(const float* x, int64_t n,
                    cvk_v view,
                    const unsigned* counts, void* stream);
int         cvk_nothing(void);
const char* cvk_text(void);
void*       cvk_handle(void* stream);
void        cvk_quiet(double a, unsigned b, long c, size_t d, uint64_t e, int32_t f, float g, const cvk_rec* r);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_on_synthetic_snippets():
    from ctypes import (c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_long, c_size_t, c_uint, c_uint8, c_uint64, c_ulonglong,
                        c_void_p)
    from pytorch_camvid_amd import _header
    h = _header.parse(SNIPPET)
    assert h.defines == {"CVK_A": 7, "CVK_B": -3, "CVK_C": -4, "CVK_D": 12, "CVK_E": 16}          # X_H, the string and the expression: skipped
    V, R = h.structs["cvk_v"], h.structs["cvk_rec"]
    assert list(h.structs) == ["cvk_v", "cvk_rec"] and issubclass(V, ctypes.Structure)
    assert V._fields_ == [("ptr", c_void_p), ("sN", c_int64), ("sY", c_int64), ("sX", c_int64)]
    assert [(n, t) for n, t in R._fields_] == [("n", c_ulonglong), ("x", c_uint8 * 256), ("rows", c_int), ("cols", c_int * 3), ("tile", c_int),
                                               ("p", c_void_p), ("inner", V)]
    assert (R.x.offset, R.rows.offset, R.cols.offset, R.tile.offset, R.p.offset, R.inner.offset) == (8, 264, 268, 280, 288, 296)
    assert ctypes.sizeof(R) == 328
    assert h.prototypes == {
        "cvk_three_lines": (c_int, [c_void_p, c_int64, V, c_void_p, c_void_p]),
        "cvk_nothing": (c_int, []),
        "cvk_text": (c_char_p, []),
        "cvk_handle": (c_void_p, [c_void_p]),
        "cvk_quiet": (None, [c_double, c_uint, c_long, c_size_t, c_uint64, c_int32, c_float, c_void_p]),
    }


@pytest.mark.parametrize("text,names", [
    ("int cvk_bad_type(flaot x);", ["cvk_bad_type", "flaot"]),
    ("int cvk_bad_pointee(const flaot* x);", ["cvk_bad_pointee", "flaot"]),
    ("int cvk_callback(int (*fn)(int), void* stream);", ["cvk_callback", "function pointer"]),
    ("int cvk_printf(const char* fmt, ...);", ["cvk_printf", "variadic"]),
    ("typedef struct cvk_bits { unsigned a : 3; unsigned b : 5; } cvk_bits;", ["cvk_bits", "bit-field"]),
    ("typedef struct cvk_outer { struct { int a; } in; int b; } cvk_outer;", ["cvk_outer", "nested struct"]),
    ("int cvk_early(cvk_late v);\ntypedef struct cvk_late { int a; } cvk_late;", ["cvk_early", "cvk_late", "before its definition"]),
    ("int cvk_never(cvk_nowhere v, int n);", ["cvk_never", "cvk_nowhere"]),
    ("int cvk_unnamed(unsigned long);", ["cvk_unnamed"]),
    ("float* cvk_returns_pointer(void);", ["cvk_returns_pointer"]),
    ("int cvk_array(float taps[12]);", ["cvk_array"]),
    ("struct cvk_forward;", ["cvk_forward"]),
])
def test_reader_refuses_what_it_does_not_know(text, names):
    """The reader never guesses (no fall-back to c_void_p): the error names the declaration and what is wrong with it."""
    from pytorch_camvid_amd import _header
    with pytest.raises(_header.CvkError) as e:
        _header.parse(text)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def prototype_arities():
    """name -> number of top-level parameters, by splitting the comment-stripped text of include/cvk.h: no call of the reader."""
    txt = open(os.path.join(ROOT, "include", "cvk.h")).read()
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    return {name: 0 if params.strip() == "void" else params.count(",") + 1
            for name, params in re.findall(r"\b(cvk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}


def test_derived_table_against_the_real_header():
    from pytorch_camvid_amd import _header, _lib
    h = _header.read(_lib.HEADER)
    assert sorted(h.prototypes) == header_symbols()
    assert h.prototypes.keys() == _lib.SIGNATURES.keys()
    arity = prototype_arities()
    assert sorted(arity) == header_symbols()
    for name, (res, args) in _lib.SIGNATURES.items():
        assert len(args) == arity[name], (name, len(args), arity[name])
    assert len(h.structs) == 12 and len(h.defines) == 19
    for c_name, py_name in _lib._NAMES.items():                       # every public name of the binding is the derived object
        assert getattr(_lib, py_name) is (_lib._H.structs.get(c_name) or _lib._H.defines[c_name]), c_name
    assert _lib.View._fields_ == [("ptr", ctypes.c_void_p), ("sN", ctypes.c_int64), ("sY", ctypes.c_int64), ("sX", ctypes.c_int64)]
    assert _lib.SIGNATURES["cvk_zero_frame"][1][0] is _lib.View and _lib.SIGNATURES["cvk_zero_frame_bf16"][1][0] is _lib.ViewH


def test_derived_structs_and_constants_against_the_real_library():
    from pytorch_camvid_amd import _lib, meters
    lib = _lib.load()
    assert ctypes.sizeof(_lib.AugmentRecord) == lib.cvk_augment_record_bytes()
    assert ctypes.sizeof(_lib.CropRecord) == lib.cvk_crop_record_bytes() == 416
    assert lib.cvk_surface_record_slots() == meters.SURFACE_RECORD_SLOTS
    assert lib.cvk_cc_record_slots() == meters.CC_RECORD_SLOTS
    assert _lib.DEFINES["CVK_VERSION"] == lib.cvk_version()
    raw = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), names=["cvk_ce_blocks"])           # bind() on a raw handle, one name or all
    assert raw.cvk_ce_blocks.argtypes == [ctypes.c_int] and raw.cvk_ce_blocks(1025) == 2
    raw = _lib.bind(ctypes.CDLL(_lib.LIB_PATH))
    assert all(getattr(raw, n).argtypes == a and getattr(raw, n).restype is r for n, (r, a) in _lib.SIGNATURES.items())


def test_missing_header_is_a_cvk_error(tmp_path):
    from pytorch_camvid_amd import _header, _lib
    missing = tmp_path / "include" / "cvk.h"
    with pytest.raises(_lib.CvkError, match="ships with the repository") as e:
        _header.read(str(missing))
    assert str(missing) in str(e.value) and not isinstance(e.value, OSError)
    assert _header.CvkError is _lib.CvkError


def test_stale_library_is_refused(tmp_path):
    """The library carries the hash of the header it was compiled against; load() compares it with the header it sees.  A library
    built from any other header (same symbol names, other argument lists) must not load."""
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    assert lib.cvk_abi_hash() == _lib.header_abi_hash()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    _lib.check_abi(raw)                                   # the real pair passes
    other = tmp_path / "cvk.h"
    other.write_bytes(open(_lib.HEADER, "rb").read() + b"\n/* one more argument somewhere */\n")
    with pytest.raises(_lib.CvkError, match="another include/cvk.h"):
        _lib.check_abi(raw, header=str(other))

    class NoStamp:                                        # a library from before the stamp existed
        pass
    with pytest.raises(_lib.CvkError, match="predates the ABI stamp"):
        _lib.check_abi(NoStamp())


def test_integration_doc_matches_the_header():
    """INTEGRATION.md is the binding guide a maintainer reads: every cvk_* name it mentions must exist in include/cvk.h, every
    entry point of the header must be mentioned, and the stated counts (entry points, .hip files) must be the real ones."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    syms = set(header_symbols())
    mentioned = set(re.findall(r"\b(cvk_[a-z0-9_]+)\b", doc)) - {"cvk_view"}          # cvk_view is the struct type
    assert not (mentioned - syms), f"INTEGRATION.md names entry points that do not exist: {sorted(mentioned - syms)}"
    assert not (syms - mentioned), f"entry points missing from INTEGRATION.md: {sorted(syms - mentioned)}"
    m = re.search(r"declares (\d+) `extern \"C\"` entry points", doc)
    assert m and int(m.group(1)) == len(syms), (m and m.group(1), len(syms))
    words = {8: "eight", 9: "nine", 10: "ten", 11: "eleven", 12: "twelve", 13: "thirteen", 14: "fourteen", 15: "fifteen"}
    nhip = len([f for f in os.listdir(os.path.join(ROOT, "pytorch-camvid_amd", "csrc")) if f.endswith(".hip")])
    assert f"{words[nhip]} `.hip` files" in doc, nhip
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"`include/cvk.h` \((\d+) entry points\)", design)
    assert m and int(m.group(1)) == len(syms), (m and m.group(1), len(syms))


def test_argument_validation_without_gpu():
    """Argument errors are detected before any launch, return CVK_EINVAL and set the error string."""
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    rc = lib.cvk_conv3x3_fwd(None, None, None, None, None, 1, 8, 8, 4, 8, 8, None)
    assert rc == -1 and b"null" in lib.cvk_last_error_string()
    rc = lib.cvk_conv3x3_fwd(16, 16, None, 16, None, 1, 8, 8, 3, 8, 8, None)
    assert rc == -1 and b"multiple of 4" in lib.cvk_last_error_string()
    assert lib.cvk_conv3x3_wgrad_workspace_bytes(8, 360, 480, 64, 64) > 0
    assert lib.cvk_bn_bwd_blocks(1382400) == 512 and lib.cvk_ce_blocks(1025) == 2


def test_module_surface_matches_reference_and_fails_loudly_on_cpu():
    import torch
    import pytorch_camvid_amd as A
    net = A.get_model("unet", 3, 12)
    assert len(net.state_dict()) == 161 and sum(p.numel() for p in net.parameters()) == 34533924
    seg = A.get_model("segnet", 3, 12)
    assert len(seg.state_dict()) == 182 and sum(p.numel() for p in seg.parameters()) == 29449956
    with pytest.raises(ValueError):
        A.get_model("nope", 3, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 3, 32, 32))
    # checkpoints interchange with the reference layout: plain OIHW tensors load into channels_last storage
    from oracle import torch_ref as R
    torch.manual_seed(3)
    ref = R.build("unet", 3, 12)
    net.load_state_dict(ref.state_dict())
    for (k, a), (_, b) in zip(net.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k
    ref.load_state_dict(net.state_dict())


def test_product_library_reads_no_environment():
    """a stray variable in a user's environment must not be able to change a kernel — least of all select one of the
    wrong-result ablation variants the timing experiments use.  Those (and every CVK_* switch of the C side) are compiled only with
    -DCVK_EXPERIMENTS into lib/libcvk_exp.so (`make experiments`, loaded by tools/ through CVK_LIB_PATH).  The product library must
    not import getenv and must not contain a CVK_* name, a *_DBG name in particular."""
    import subprocess
    from pytorch_camvid_amd import _lib
    path = os.path.join(ROOT, "pytorch-camvid_amd", "lib", "libcvk.so")
    if not os.path.exists(path):
        _lib.build()
    data = open(path, "rb").read()
    names = sorted(set(m.decode() for m in re.findall(rb"CVK_[A-Z0-9_]{3,}", data)))
    assert not [n for n in names if n.endswith("_DBG")], names
    assert not names, f"environment-style names inside the product library: {names}"
    undefined = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined, "libcvk.so imports getenv"
    # and the superseded kernel generations are gone from the default build (they live in git history)
    assert b"k_conv_bf16p" not in data and b"k_wgrad_bf16sI" not in data
    # the product never loads the experiments build by itself: only an explicit CVK_LIB_PATH does
    assert _lib.LIB_PATH == (os.environ.get("CVK_LIB_PATH") or path)
