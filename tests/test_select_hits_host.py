"""The hit selection's specification (gnn-fpga_amd/select_hits.py) against the reference's own select_hits
(tests/golden/select_hits, written by tools/gen_select_hits_golden.py running gnn/prepareGraphs.py:53-85 per event),
the chain into build_graphs against the reference's graphs, the stated differences, input validation and the C ABI's
new entry points; no GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

from gnn_fpga_amd import BARREL_VLIDS, SelectedHits, _lib, select_hits, synth
from select_hits_fixtures import (CASES, GOLD, assert_equals_reference, assert_graphs_equal, assert_same,
                                  chain_reference_batch, load, select, tables)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2 ** 62


def test_fixtures_cover_the_cases():
    assert set(CASES) >= {"default", "no_missing", "ties", "pt_edge", "pt_edge_zero", "ids", "other_volumes",
                          "multi_event", "chain"}
    rec = json.load(open(os.path.join(GOLD, "reference_time.json")))
    assert rec["hits"] > 100000 and rec["seconds"] > 0
    for c in CASES:
        size = os.path.getsize(os.path.join(GOLD, c + ".npz"))
        assert size < 100000, (c, size)
        f = load(c)
        for e in range(len(f["hits_event_ptr"]) - 1):                       # every barrel layer has rows in every event
            s = slice(f["hits_event_ptr"][e], f["hits_event_ptr"][e + 1])
            assert set(zip(f["hits_volume_id"][s].tolist(), f["hits_layer_id"][s].tolist())) >= set(BARREL_VLIDS)


@pytest.mark.parametrize("case", CASES)
def test_specification_equals_the_reference(case):
    f = load(case)
    sel = select(f)
    assert isinstance(sel, SelectedHits) and sel.r.device.type == "cpu" and len(sel) > 0
    assert_equals_reference(sel, f)
    assert_equals_reference(select(f, phi=False), f, phi=False)          # (np.arctan2 here, as in the reference)
    assert np.array_equal(select(f, phi=False).phi.numpy().view(np.uint32), f["ref_phi"].view(np.uint32))


def test_fixture_traps_are_present():
    """The cases pin what they are named for."""
    f = load("no_missing")
    assert bool(f["no_missing_hits"]) and len(select(f, no_missing_hits=False)) > len(select(f))
    f = load("ties")
    r = np.sqrt(f["hits_x"] ** 2 + f["hits_y"] ** 2)
    lay = {vl: k for k, vl in enumerate(BARREL_VLIDS)}
    tp = dict(zip(f["truth_hit_id"].tolist(), f["truth_particle_id"].tolist()))
    groups = {}
    for q in range(r.shape[0]):
        key = (tp.get(int(f["hits_hit_id"][q])), lay.get((int(f["hits_volume_id"][q]), int(f["hits_layer_id"][q]))))
        groups.setdefault(key, []).append(q)
    n_big = 0
    for row, pid, l in zip(f["ref_row"], f["ref_particle_id"], f["ref_layer"]):
        g = groups[(int(pid), int(l))]
        least = [q for q in g if r[q] == min(r[k] for k in g)]
        assert row == min(least)
        n_big += len(least) >= 3
    assert n_big >= 10
    f = load("pt_edge")
    pt = np.sqrt(f["particles_px"] ** 2 + f["particles_py"] ** 2)
    assert pt.dtype == np.float32
    edge = f["particles_particle_id"][pt == np.float32(f["pt_min"])]
    assert edge.size == 1 and edge[0] not in f["ref_particle_id"] and edge[0] in f["truth_particle_id"]
    assert edge[0] in select(f, pt_min=float(np.nextafter(np.float32(f["pt_min"]), np.float32(0)))).particle_id
    f = load("pt_edge_zero")
    zero = f["particles_particle_id"][(f["particles_px"] == 0) & (f["particles_py"] == 0)]
    assert float(f["pt_min"]) == 0.0 and zero.size == 1 and zero[0] not in f["ref_particle_id"]
    f = load("ids")
    got = set(f["ref_particle_id"].tolist())
    assert {BIG + 1, BIG + 5, BIG + 6} <= got and BIG + 2 not in got    # one apart above 2^53: still distinct
    assert float(BIG + 1) == float(BIG + 2)
    assert not np.isin(f["truth_hit_id"], f["hits_hit_id"]).all() and not np.isin(f["hits_hit_id"], f["truth_hit_id"]).all()
    assert not np.isin(f["particles_particle_id"], f["truth_particle_id"]).all()
    f = load("other_volumes")
    assert {(8, 3), (7, 2), (9, 4)} <= set(zip(f["hits_volume_id"].tolist(), f["hits_layer_id"].tolist()))
    f = load("multi_event")
    ep, hp, pp = f["ref_event_ptr"], f["hits_event_ptr"], f["particles_event_ptr"]
    assert len(ep) == 4 and ep[1] == ep[2] and 0 < ep[1] < ep[3]
    assert all(f["hits_hit_id"][hp[e]:hp[e + 1]].min() == 1 for e in range(3))
    assert set(f["particles_particle_id"][pp[0]:pp[1]].tolist()) & set(f["particles_particle_id"][pp[2]:pp[3]].tolist())


def test_output_order_and_columns():
    f = load("multi_event")
    sel = select(f)
    row = sel.row.numpy()
    assert np.array_equal(sel.hit_id.numpy(), f["hits_hit_id"][row]) and np.array_equal(sel.z.numpy(), f["hits_z"][row])
    assert np.array_equal(sel.phi.numpy(), f["phi"][row])
    evt = np.repeat(np.arange(3), np.diff(f["hits_event_ptr"]))
    assert np.array_equal(evt[row], np.repeat(np.arange(3), np.diff(sel.event_ptr)))
    for a, b in zip(sel.event_ptr[:-1], sel.event_ptr[1:]):
        k = np.stack([sel.particle_id.numpy()[a:b], sel.layer.numpy()[a:b]], axis=1)
        assert np.array_equal(k, k[np.lexsort((k[:, 1], k[:, 0]))]) and len(np.unique(k, axis=0)) == b - a


def test_chain_equals_the_reference_graphs():
    f = load("chain")
    psm, pso, z0m = (float(c) for c in f["cuts"])
    sel = select(f)
    b = sel.build_graphs(n_phi_sectors=int(f["n_phi_sectors"]), phi_slope_max=psm, phi_slope_outer_max=pso, z0_max=z0m)
    ref = chain_reference_batch(f)
    assert b.n_graphs == 2 * int(f["n_phi_sectors"]) and b.n_segments > 100
    assert_graphs_equal(b, ref)
    assert np.array_equal(sel.row.numpy()[b.hit_index.numpy()], f["ref_row"][b.hit_index.numpy()])
    pairs = np.stack([np.arange(9), np.arange(1, 10)], axis=1)
    assert_graphs_equal(sel.build_graphs(layer_pairs=pairs, n_phi_sectors=8), ref)         # the default pairs and cuts


def test_a_barrel_layer_without_rows_gives_no_hits_on_it():
    """Where the reference raises KeyError from get_group: the specification only."""
    f = load("default")
    h, t, p = tables(f)
    keep = ~((h["volume_id"] == 13) & (h["layer_id"] == 4))
    cut = {k: (v if k == "event_ptr" else v[keep]) for k, v in h.items()}
    cut["event_ptr"] = np.array([0, int(keep.sum())])
    sel = select_hits(cut, t, p, pt_min=0.5, phi=f["phi"][keep])
    assert 5 not in sel.layer.tolist() and set(sel.layer.tolist()) == set(range(10)) - {5}
    m = f["ref_layer"] != 5
    assert np.array_equal(np.flatnonzero(keep)[sel.row.numpy()], f["ref_row"][m])
    assert np.array_equal(sel.r.numpy().view(np.uint32), f["ref_r"][m].view(np.uint32))
    assert len(select_hits(cut, t, p, pt_min=0.5, no_missing_hits=True)) == 0


def test_barrel_layers_argument_and_no_missing_hits_count():
    f = load("default")
    three = ((17, 4), (8, 2), (13, 2))                                  # any list: the layer is the index in it
    sel = select(f, barrel_layers=three)
    full = select(f)
    for k, l in enumerate((9, 0, 4)):
        assert np.array_equal(np.sort(sel.row.numpy()[sel.layer.numpy() == k]),
                              np.sort(full.row.numpy()[full.layer.numpy() == l]))
    nm = select(f, barrel_layers=three, no_missing_hits=True)           # len(barrel_layers) layers, not 10
    pid, cnt = np.unique(nm.particle_id.numpy(), return_counts=True)
    assert 0 < len(nm) < len(sel) and np.all(cnt == 3)
    assert_same(select(f, barrel_layers=BARREL_VLIDS + ((8, 2),)), full)        # a repeated pair: the first index
    for bad in ((), [(1, 2)] * 65, [(2 ** 31, 1)]):
        with pytest.raises(ValueError, match="barrel_layers"):
            select(f, barrel_layers=bad)


def test_input_refusals():
    f = load("multi_event")
    for tb, col in ((0, "x"), (0, "y"), (0, "z"), (2, "px"), (2, "py")):
        tabs = tables(f)
        tabs[tb][col] = tabs[tb][col].astype(np.float64)
        with pytest.raises(ValueError, match="float64: the reference's selection is float32 arithmetic"):
            select_hits(*tabs)
    with pytest.raises(ValueError, match="phi must be a float32"):
        select_hits(*tables(f), phi=f["phi"].astype(np.float64))
    with pytest.raises(ValueError, match="phi has"):
        select_hits(*tables(f), phi=f["phi"][:-1])
    for tb, col in ((0, "hit_id"), (1, "hit_id"), (2, "particle_id")):          # twice in ONE event's table
        tabs = tables(f)
        ep = tabs[tb]["event_ptr"]
        tabs[tb][col] = tabs[tb][col].copy()
        tabs[tb][col][ep[2] + 3] = tabs[tb][col][ep[2] + 7]
        with pytest.raises(ValueError, match="duplicated"):
            select_hits(*tabs)
    for col, v in (("x", np.nan), ("y", np.inf), ("x", -np.inf)):
        tabs = tables(f)
        tabs[0][col] = tabs[0][col].copy()
        tabs[0][col][5] = v
        with pytest.raises(ValueError, match="non-finite"):
            select_hits(*tabs)
    for tb in range(3):
        ep = f["%s_event_ptr" % ("hits", "truth", "particles")[tb]]
        for bad in (ep[::-1].copy(), ep[:-1], ep + 1, np.array([0]), ep.astype(np.float32)):
            tabs = tables(f)
            tabs[tb]["event_ptr"] = bad
            with pytest.raises(ValueError, match="event_ptr"):
                select_hits(*tabs)
    tabs = tables(f)
    del tabs[1]["particle_id"]
    with pytest.raises(ValueError, match="particle_id"):
        select_hits(*tabs)
    tabs = tables(f)
    tabs[0]["volume_id"] = tabs[0]["volume_id"].astype(np.float32)
    with pytest.raises(ValueError, match="integer"):
        select_hits(*tabs)
    tabs = tables(f)
    tabs[1]["hit_id"] = tabs[1]["hit_id"][:-1]
    with pytest.raises(ValueError, match="entries"):
        select_hits(*tabs)
    with pytest.raises(ValueError, match="NaN"):
        select_hits(*tables(f), pt_min=float("nan"))
    t = torch.from_numpy
    tabs = [{k: (v if k == "event_ptr" else t(v)) for k, v in tb.items()} for tb in tables(f)]     # CPU tensors
    assert_same(select_hits(*tabs, pt_min=0.5, phi=t(f["phi"])), select(f))


def test_empty_inputs_and_synthetic_events():
    none = {"hit_id": np.zeros(0, np.int32), "x": np.zeros(0, np.float32), "y": np.zeros(0, np.float32),
            "z": np.zeros(0, np.float32), "volume_id": np.zeros(0, np.int32), "layer_id": np.zeros(0, np.int32)}
    sel = select_hits(none, {"hit_id": np.zeros(0, np.int64), "particle_id": np.zeros(0, np.int64)},
                      {"particle_id": np.zeros(0, np.int64), "px": np.zeros(0, np.float32), "py": np.zeros(0, np.float32)})
    assert len(sel) == 0 and sel.event_ptr.tolist() == [0, 0] and sel.r.dtype == torch.float32
    assert sel.build_graphs(n_phi_sectors=2).n_hits == 0
    ev = synth.trackml_events(3, 30, 40, seed=3)
    every = select_hits(ev["hits"], ev["truth"], ev["particles"])
    some = select_hits(ev["hits"], ev["truth"], ev["particles"], pt_min=1.0)
    nm = select_hits(ev["hits"], ev["truth"], ev["particles"], pt_min=1.0, no_missing_hits=True)
    assert len(every) > len(some) > len(nm) > 0 and set(nm.row.tolist()) <= set(some.row.tolist()) <= set(every.row.tolist())
    assert 0 not in every.particle_id.tolist()


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "gnn_hip.h")) as fh:
        hdr = fh.read()
    names = ("gnn_select_hits_workspace_bytes", "gnn_select_hits_sizes", "gnn_select_hits_fill")
    for n in names:
        assert re.search(r"\b%s\(" % n, hdr) and n in _lib.SIGNATURES
    assert "GNN_ABI_VERSION 7" in hdr and _lib.GNN_ABI_VERSION == 7
    doc = hdr.split("csrc/select_hits.hip; ABI 7")[1].split("gnn_select_hits_fill(")[0]
    for cite in ("gnn/prepareGraphs.py:53-85", ":64-67", ":68-69", ":74-76", ":77-80", ":82-84"):
        assert cite in doc                                             # the reference lines it replaces
    assert "GNN_SELECT_HITS_MAX_LAYERS %d" % _lib.SELECT_HITS_MAX_LAYERS in hdr
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gnn_abi_version() == 7
    assert lib.gnn_select_hits_workspace_bytes(100, 100, 10, 0) == 0 and "n_events" in lib.gnn_last_error().decode()
    assert lib.gnn_select_hits_workspace_bytes(-1, 1, 1, 1) == 0
    assert lib.gnn_select_hits_workspace_bytes(1, 2 ** 31, 1, 1) == 0
    assert lib.gnn_select_hits_workspace_bytes(0, 0, 0, 1) > 0
    assert lib.gnn_select_hits_workspace_bytes(1000, 900, 100, 3) > lib.gnn_select_hits_workspace_bytes(100, 90, 10, 3)
    tab = np.asarray(BARREL_VLIDS, np.int32)

    def sizes(n_layers=10, pt_min=0.5, table=tab.ctypes.data):
        return lib.gnn_select_hits_sizes(None, None, None, None, None, 10, None, None, None, 10, None, None, None, None,
                                         5, None, 1, table, n_layers, pt_min, 0, None, 0, None, None, None)
    assert sizes() == _lib.GNN_ERR_BADARG and "pointer" in lib.gnn_last_error().decode()
    assert sizes(n_layers=65) == _lib.GNN_ERR_BADARG and "barrel_layers" in lib.gnn_last_error().decode()
    assert sizes(table=None) == _lib.GNN_ERR_BADARG and "barrel_layers" in lib.gnn_last_error().decode()
    assert sizes(pt_min=float("nan")) == _lib.GNN_ERR_BADARG and "NaN" in lib.gnn_last_error().decode()

    def fill(s):
        return lib.gnn_select_hits_fill(None, None, None, None, None, 100, 100, 10, 1, 0, s, None, 0, *([None] * 8))
    assert fill(_lib.GnnSelectHitsSizes(n_kept=5, status=16)) == _lib.GNN_ERR_BADARG
    assert "flagged" in lib.gnn_last_error().decode()
    assert fill(_lib.GnnSelectHitsSizes(n_kept=500)) == _lib.GNN_ERR_BADARG
    assert fill(_lib.GnnSelectHitsSizes(n_kept=5)) == _lib.GNN_ERR_BADARG and "pointer" in lib.gnn_last_error().decode()
    assert fill(_lib.GnnSelectHitsSizes(n_kept=0)) == 0


def test_units_name_select_hits():
    from variant_scripts import assert_variant_libraries_link
    assert_variant_libraries_link("select_hits")
    with open(os.path.join(REPO, "gnn-fpga_amd", "csrc", "select_hits.hip")) as fh:
        src = fh.read()
    assert "#pragma clang fp contract(off)" in src and '#include "builder_sort.h"' in src
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "builder_sort.h"')


def test_new_kernels_have_no_scratch():
    path = os.path.join(REPO, "build", "select_hits.remarks")
    if not os.path.exists(path):
        pytest.fail("build/select_hits.remarks is missing: build the library first")
    with open(path) as fh:
        text = fh.read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    ours = [b for b in blocks if "k_sh_" in b.split()[0]]
    assert len(ours) >= 13                                        # thirteen kernels
    for b in ours:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split()[0]
