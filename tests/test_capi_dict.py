"""bic_dict_encode / bic_set_dict_block exist at every layer and reject bad arguments before any device work
(CPU only: every call here returns BIC_EINVAL from its argument checks; the context pointer of the calls that
pass a non-null one is never dereferenced, because an argument is wrong)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pybic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def call(ctx, variant=3, W=16, atom_step=1, rows=64, cols=64, wpr=1, plane=True, enuml=True, stats=True,
         streams=False, cap_words=0):
    lib = pybic.load()
    buf = np.zeros(4096, np.uint64)
    e = np.zeros(64 * 64 + 1, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    return lib.bic_dict_encode(ctx, variant, p if plane else None, rows, cols, wpr, W, 0, atom_step,
                               e.ctypes.data_as(C.c_void_p) if enuml else None, None, None, None, None, None, None,
                               None, p if streams else None, p if streams else None, cap_words, p if stats else None)


@pytest.fixture()
def fake_ctx():
    mem = (C.c_char * 4096)()  # never read: the argument checks come first
    yield C.cast(mem, C.c_void_p)


def test_null_ctx():
    assert call(None) == pybic.BIC_EINVAL
    assert pybic.load().bic_set_dict_block(None, 4) == pybic.BIC_EINVAL


@pytest.mark.parametrize("kw", [dict(W=0), dict(W=65), dict(variant=4), dict(variant=0), dict(W=16, atom_step=2),
                                dict(W=16, atom_step=0), dict(W=8, atom_step=16), dict(plane=False),
                                dict(enuml=False), dict(stats=False), dict(cols=0), dict(cols=65, wpr=1),
                                dict(streams=True, cap_words=0), dict(streams=False, cap_words=8)])
def test_einval_without_a_device(fake_ctx, kw):
    assert call(fake_ctx, **kw) == pybic.BIC_EINVAL


def test_declared_exported_bound():
    src = open(os.path.join(ROOT, "include", "bic.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bic_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}
    assert len(decl["bic_dict_encode"].split(",")) == 21 and len(decl["bic_set_dict_block"].split(",")) == 2
    lib = pybic.load()
    assert len(lib.bic_dict_encode.argtypes) == 21 and len(lib.bic_set_dict_block.argtypes) == 2
    assert {"bic_dict_encode", "bic_set_dict_block"} <= set(pybic.EXPORTS)
    assert callable(getattr(pybic.Context, "dict_encode", None)) and callable(getattr(pybic.Context, "set_dict_block", None))
