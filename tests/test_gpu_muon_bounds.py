"""The muon graph builder on the GPU at the bounds its kernels are written for (tests/muon_bound_cases.py): one batch
of every case, built flat, padded, and padded followed by check(), against the specification on the same input bit
for bit; then what the cases claim read off the device's own arrays: the pair order against the interpreter's set, the
l1-major segment order, the cut decisions, the slots beside the full entry."""
import functools

import numpy as np
import pytest
import torch

import muon_bound_cases as mb
from gnn_fpga_amd import build_muon_graphs
from test_gpu_muon_graph import _dev, _host, _vp, assert_same

pytestmark = pytest.mark.gpu

START = 3


@functools.lru_cache(maxsize=None)
def spec(layout):
    mu, pu, vpt, veta = mb.batch_columns()
    return build_muon_graphs(mu, pu, vpt, veta, entry_start=START, layout=layout)


@functools.lru_cache(maxsize=None)
def device_args():
    mu, pu, vpt, veta = mb.batch_columns()
    return _dev(mu), _dev(pu), *_vp(vpt, veta)


@functools.lru_cache(maxsize=None)
def device(layout):
    return _host(build_muon_graphs(*device_args(), entry_start=START, layout=layout))


@pytest.mark.parametrize("layout", ["flat", "padded"])
def test_device_matches_spec_on_every_bound_case(layout):
    got = device(layout)
    assert_same(got, spec(layout))
    assert got.n_hits.max() == 42 and got.n_segments.max() == 140


def test_padded_then_check():
    res = build_muon_graphs(*device_args(), entry_start=START, layout="padded")
    assert res.check() is res and int(res.status.cpu()[0]) == 0
    assert_same(_host(res), spec("padded"))


@pytest.mark.parametrize("layout", ["flat", "padded"])
def test_device_orders_are_the_interpreters(layout):
    top = mb.check_cases(device(layout))
    assert top == dict(hits=42, layer_hits=6, distinct=25, candidates=140, rounds=3, rows=320), top


def test_nothing_leaks_into_the_slots_beside_a_full_entry():
    def build(entries):
        mu, pu, vpt, veta = mb.columns(entries)
        return _host(build_muon_graphs(_dev(mu), _dev(pu), *_vp(vpt, veta), layout="padded"))

    mb.check_neighbours(device("padded"), build)
    torch.cuda.synchronize()
