"""tests/poisoned_alloc.py on CPU tensors: the views it hands out, the two patterns, what the guard check sees and
names, what the proxy leaves alone, that the patch is undone - and that its module list misses no allocating module
of the package."""
import glob
import os
import types

import numpy as np
import pytest
import torch

from poisoned_alloc import ALIGN, GUARD, MODULES, poison

HERE = os.path.abspath(__file__)

SHAPES = [(3, 5), (7,), (0,), (13,), (1,), (2, 0, 3), (257, 3)]
DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32, torch.bfloat16]


def _module():
    """A stand-in for one of the package's modules: a namespace whose `torch` the helper replaces."""
    return types.ModuleType("poisoned_alloc_victim")


@pytest.fixture()
def mod():
    m = _module()
    m.torch = torch
    return m


def _line():
    import sys
    return sys._getframe(1).f_lineno


def test_guard_is_the_condition_the_issue_sets():
    assert GUARD >= 64 * 1024 and GUARD % 512 == 0 and ALIGN == 512


@pytest.mark.parametrize("pattern", ["ff", "one"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_views(mod, pattern, dtype, shape):
    with poison(pattern, modules=[mod], devices=("cpu",)) as p:
        forms = [mod.torch.empty(shape, dtype=dtype), mod.torch.empty(*shape, dtype=dtype, device="cpu"),
                 mod.torch.empty_like(torch.zeros(shape, dtype=dtype)),
                 mod.torch.empty_like(torch.zeros(shape), dtype=dtype, device=torch.device("cpu"))]
        for t in forms:
            assert t.shape == torch.Size(shape) and t.dtype == dtype and t.device.type == "cpu"
            assert t.is_contiguous() and t.data_ptr() % 512 == 0
        assert len(p.records) == len(forms)
        for (block, nbytes, _), t in zip(p.records, forms):
            assert block.dtype == torch.uint8 and nbytes == t.numel() * t.element_size()
            assert block.numel() == GUARD + (nbytes + 7) // 8 * 8 + GUARD
            es = t.element_size()                # (data_ptr() of a 0-size tensor is 0: ask the storage)
            assert t.untyped_storage().data_ptr() + t.storage_offset() * es == block.data_ptr() + GUARD
        # an in-bounds write of every element leaves the guards intact
        for t in forms:
            t.zero_()
        assert p.guards_intact() == []


def test_default_dtype_and_device(mod):
    with poison("ff", modules=[mod], devices=("cpu",)) as p:
        t = mod.torch.empty(4)
        assert t.dtype == torch.get_default_dtype() and len(p.records) == 1


def test_pattern_ff_reads_back_as_documented(mod):
    with poison("ff", modules=[mod], devices=("cpu",)):
        assert torch.isnan(mod.torch.empty(9, dtype=torch.float32)).all()
        assert torch.isnan(mod.torch.empty(9, dtype=torch.float64)).all()
        assert torch.isnan(mod.torch.empty(9, dtype=torch.bfloat16).float()).all()
        assert (mod.torch.empty(9, dtype=torch.int32) == -1).all()
        assert (mod.torch.empty(9, dtype=torch.int64) == -1).all()
        assert (mod.torch.empty(13, dtype=torch.uint8) == 255).all()


def test_pattern_one_reads_back_as_documented(mod):
    with poison("one", modules=[mod], devices=("cpu",)):
        assert (mod.torch.empty(9, dtype=torch.int64) == 1).all()
        assert mod.torch.empty(9, dtype=torch.int32).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1]
        assert mod.torch.empty(13, dtype=torch.uint8).tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
        f = mod.torch.empty(9, dtype=torch.float32)
        tiny = float(np.finfo(np.float32).tiny)
        assert ((f == 0) | ((f > 0) & (f < tiny))).all()                    # denormal or 0
        d = mod.torch.empty(9, dtype=torch.float64)
        assert ((d > 0) & (d < float(np.finfo(np.float64).tiny))).all()
        assert ((mod.torch.empty(9, dtype=torch.bfloat16).float().abs()) < tiny).all()


@pytest.mark.parametrize("pattern", ["ff", "one"])
@pytest.mark.parametrize("where", [-1, 1], ids=["before", "after"])
@pytest.mark.parametrize("dtype,shape", [(torch.float32, (3, 5)), (torch.int64, (7,)), (torch.int32, (0,)),
                                         (torch.uint8, (13,)), (torch.bfloat16, (5,))], ids=str)
def test_overrun_is_reported_with_its_call_site(mod, pattern, where, dtype, shape):
    with poison(pattern, modules=[mod], devices=("cpu",)) as p:
        a = mod.torch.empty(5, dtype=torch.float32)
        t = mod.torch.empty(shape, dtype=dtype); line = _line()
        b = mod.torch.empty_like(a)
        a.fill_(2.0), t.fill_(3), b.fill_(4.0)
        assert p.guards_intact() == []
        block, nbytes, site = p.records[1]
        assert site == "%s:%d" % (HERE, line)
        es = t.element_size()
        at = GUARD - es if where < 0 else GUARD + nbytes
        if pattern == "one" and not block[at:at + es].any():
            # the documented blind spot: zeros written into zero bytes; a nonzero value is still seen
            block[at:at + es] = 0
            assert p.guards_intact() == []
            block[at:at + es] = 7
        else:
            block[at:at + es] = 0
        assert p.guards_intact() == [site]
        # the neighbours' guards are their own
        assert (a == 2.0).all() and (b == 4.0).all()


def test_far_edges_of_the_guards_are_checked(mod):
    with poison("ff", modules=[mod], devices=("cpu",)) as p:
        mod.torch.empty(3, dtype=torch.int32)
        block, _, site = p.records[0]
        block[0] = 0
        assert p.guards_intact() == [site]
        block[0] = 255
        assert p.guards_intact() == []
        block[-1] = 0
        assert p.guards_intact() == [site]


def test_other_devices_and_unknown_keywords_go_to_the_real_function(mod):
    with poison("ff", modules=[mod], devices=("cuda",)) as p:
        mod.torch.empty(4), mod.torch.empty_like(torch.zeros(4))            # CPU allocations: not ours
        assert p.records == []
    with poison("ff", modules=[mod], devices=("cpu",)) as p:
        t = mod.torch.empty(4, pin_memory=False)
        u = mod.torch.empty_like(torch.zeros(2, 3), memory_format=torch.contiguous_format)
        assert p.records == [] and t.shape == (4,) and u.shape == (2, 3)


def test_every_other_attribute_is_the_real_one(mod):
    with poison("ff", modules=[mod], devices=("cpu",)) as p:
        assert mod.torch is p.proxy and mod.torch is not torch
        for name in ("zeros", "zeros_like", "full", "tensor", "float32", "int64", "nn", "cuda", "Tensor", "device",
                     "no_grad", "from_numpy", "autograd", "distributed", "ones", "arange"):
            assert getattr(mod.torch, name) is getattr(torch, name), name
        assert mod.torch.empty is not torch.empty and mod.torch.empty_like is not torch.empty_like
        z = mod.torch.zeros(5)
        assert (z == 0).all() and p.records == []
        with pytest.raises(AttributeError):
            mod.torch.no_such_attribute


def test_patch_is_undone_on_exit_and_after_an_exception(mod):
    other = _module()                        # a module without the name `torch` is left without it
    with poison("one", modules=[mod, other], devices=("cpu",)) as p:
        assert mod.torch is p.proxy
    assert mod.torch is torch and not hasattr(other, "torch") and p.records == []
    with pytest.raises(ZeroDivisionError):
        with poison("ff", modules=[mod], devices=("cpu",)):
            assert mod.torch is not torch
            1 / 0
    assert mod.torch is torch


def test_the_package_is_patched_and_restored():
    import importlib
    mods = [importlib.import_module("gnn_fpga_amd." + m) for m in MODULES]
    assert all(m.torch is torch for m in mods)
    with poison("ff") as p:
        assert all(m.torch is p.proxy for m in mods)
    assert all(m.torch is torch for m in mods)


def test_module_list_misses_no_allocating_module():
    """A source scan, so that a new module cannot slip past: every .py of the package that allocates uninitialised
    (or through a tensor's new_* methods) is in the helper's list."""
    import gnn_fpga_amd
    needles = ("torch.empty(", "torch.empty_like(", ".new_empty(", ".new_zeros(")
    found = set()
    files = sorted(glob.glob(os.path.join(gnn_fpga_amd.__path__[0], "**", "*.py"), recursive=True))
    assert len(files) > 20
    for path in files:
        with open(path) as f:
            text = f.read()
        if any(n in text for n in needles):
            rel = os.path.relpath(path, gnn_fpga_amd.__path__[0])[:-3].replace(os.sep, ".")
            found.add(rel[:-len(".__init__")] if rel.endswith(".__init__") else rel)
    assert "_lib" in found                    # the scan sees what it is for
    assert found <= set(MODULES), "allocating modules poisoned_alloc.MODULES lacks: %s" % sorted(found - set(MODULES))
    assert len(set(MODULES)) == len(MODULES) == 10
