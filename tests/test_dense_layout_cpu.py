"""The host-visible surface of the opt-in dense layout (variant 6 / block variant 3): the C declaration, the ctypes
prototype, the variant tables, ``from_dense``'s ``layout`` argument and the byte count the bench tool divides by.  No GPU:
the operator methods are called on a stub that carries the sizes only."""
import inspect
import os
import re
import types

from conftest import REPO
from eigensolvers_amd import _lib
from eigensolvers_amd.hip_vector import HipCsrOperator


def test_header_declares_dense_info_and_lib_prototypes_it():
    header = open(os.path.join(REPO, "include", "hipeig.h")).read()
    assert re.search(r"int\s+hipeig_csr_dense_info\s*\(\s*hipeig_csr\s*\*\s*A\s*,\s*int64_t\s+out\[8\]\s*\)\s*;", header)
    assert "numpyVector.py:100" in header and ":152" in header          # the reference call sites it serves
    assert _lib.SIGNATURES["hipeig_csr_dense_info"] == _lib.SIGNATURES["hipeig_csr_pair_info"]      # (handle, int64*)


def test_variant_tables_name_the_dense_layout():
    assert HipCsrOperator.VARIANTS[6] == "dense" and HipCsrOperator.BLOCK_VARIANTS[3] == "dense"
    assert sorted(HipCsrOperator.VARIANTS) == list(range(7)) and sorted(HipCsrOperator.BLOCK_VARIANTS) == list(range(4))
    assert "6" in HipCsrOperator.set_variant.__doc__ and "dense" in HipCsrOperator.set_variant.__doc__


def test_from_dense_takes_a_layout_that_defaults_to_none():
    p = inspect.signature(HipCsrOperator.from_dense).parameters
    assert list(p) == ["M", "ctx", "layout"] and p["layout"].default is None and p["ctx"].default is None


def test_dense_algorithmic_bytes_on_a_stub_of_the_sizes():
    for nrows, ncols in ((1, 1), (100, 100), (8192, 8192), (3, 5)):
        stub = types.SimpleNamespace(nrows=nrows, ncols=ncols)
        assert HipCsrOperator.dense_algorithmic_bytes(stub) == 8 * nrows * ncols + 8 * ncols + 8 * nrows
    assert HipCsrOperator.dense_algorithmic_bytes(types.SimpleNamespace(nrows=8192, ncols=8192)) == 536_870_912 + 2 * 65_536
