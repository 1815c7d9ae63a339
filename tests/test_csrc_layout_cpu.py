"""The layout of csrc/loss_eval_optim.hip: every subject is a per-subject header that the file includes, and the file itself keeps
only the library-wide pieces.  Every header it includes must compile on its own (its own includes, its own namespace, no dependence
on where it is included), and the file must not grow again: it defines no kernel, opens no namespace, and its only entry points are
the version, the ABI stamp and the error string.  No GPU: the compiler only parses."""
import functools
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-camvid_amd", "csrc")
UNIT = os.path.join(CSRC, "loss_eval_optim.hip")
LIBRARY_WIDE = ["cvk_version", "cvk_abi_hash", "cvk_last_error_string"]      # the `extern "C"` definitions of the .hip, in its order


def included_headers():
    return re.findall(r'^#include "([^"]+)"', open(UNIT).read(), flags=re.M)


@functools.lru_cache(maxsize=None)
def makefile_compiler_and_flags():
    """$(HIPCC) $(FLAGS) as the Makefile expands them (the ABI stamp included)"""
    out = subprocess.run(["make", "-s", "-C", CSRC, "--no-print-directory", "--eval", "print-flags: ; @echo $(HIPCC) $(FLAGS)", "print-flags"],
                         check=True, capture_output=True, text=True).stdout
    return tuple(shlex.split(out))


def test_the_unit_includes_its_subjects():
    headers = included_headers()
    assert "cvk_common.h" in headers and "surface_dist.h" in headers and "loss_ce.h" in headers, headers
    assert len(set(headers)) == len(headers), "a header is included twice"
    head = open(UNIT).read().split("\nnamespace", 1)[0]
    assert headers == re.findall(r'^#include "([^"]+)"', head, flags=re.M), "a header is included inside a namespace"


@pytest.mark.parametrize("header", included_headers())
def test_header_compiles_alone(header):
    text = open(os.path.join(CSRC, header)).read()
    assert re.search(r"^#pragma once$", text, flags=re.M), f"{header} has no #pragma once"
    cmd = list(makefile_compiler_and_flags()) + ["-x", "hip", "-fsyntax-only", "-Wno-pragma-once-outside-header", header]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, f"{header} does not compile on its own:\n{r.stderr[-4000:]}"


def code_of_the_unit():
    return re.sub(r"//[^\n]*", "", open(UNIT).read())


def test_the_unit_grows_no_kernel():
    """A new kernel, whatever its name, goes into the header of its subject (or a new header), not into the .hip."""
    text = code_of_the_unit()
    assert text.count("__global__") == 0, "loss_eval_optim.hip defines a kernel: put it into a per-subject header"
    assert not re.search(r"\bnamespace\b", text), "loss_eval_optim.hip opens a namespace: helpers live in their subject's header"


def test_the_unit_defines_only_the_library_wide_entry_points():
    names = re.findall(r'extern\s+"C"[^;{(]*?(\w+)\s*\(', code_of_the_unit())
    assert names == LIBRARY_WIDE, f"loss_eval_optim.hip defines {names}: an entry point goes into its subject's header"
