"""What tests/test_gpu_lane_sweeps.py relies on, checked without a GPU: the graphs of tests/lane_graphs.py have the
prescribed list lengths and a plan that takes the k_iter2 route, every k_iter2 instantiation of the build has zero
scratch and no AGPRs (its prefetch keeps asm-loaded registers in flight: a spill would save garbage), and the
launch variants that score one list step per lane (csrc/sell_pipeline.hip: Cfg::lane_sweep, sweep16_lane) are the
ones profiles/lane_sweep_ab.txt measured faster."""
import os
import re
import subprocess

import numpy as np
import pytest

from gnn_fpga_amd import HitGraphBatch, _lib
from gnn_fpga_amd.plan import SellPlan

import lane_graphs
import trim_graphs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "gnn-fpga_amd", "csrc", "sell_pipeline.hip")


def test_graphs_have_the_prescribed_list_lengths():
    graphs = lane_graphs.lane_graphs(3)
    assert len(graphs) == lane_graphs.N_GRAPHS == 3
    per = lane_graphs.PER_LAYER
    for g in graphs:
        n = g.X.shape[0]
        assert n == 2560 and g.X.shape[1] == 3
        assert ((g.dst // per) - (g.src // per) == 1).all()             # consecutive layers only
        assert len(set(zip(g.src.tolist(), g.dst.tolist()))) == g.src.shape[0]
        deg_in, deg_out = np.bincount(g.dst, minlength=n), np.bincount(g.src, minlength=n)
        for deg in (deg_in[per:], deg_out[:-per]):                      # (the first layer has no in-lists, ...)
            values, counts = np.unique(deg, return_counts=True)
            assert tuple(values.tolist()) == lane_graphs.LENGTHS
            assert counts.min() >= 8


@pytest.mark.parametrize("F,D", [(3, 8), (2, 8), (3, 4), (11, 8)])
def test_plan_reaches_every_length_and_fits_k_iter2(F, D):
    batch = HitGraphBatch.from_graphs(lane_graphs.lane_graphs(F))
    plan = SellPlan(batch, _lib.plan_limits(F, D))
    for steps in trim_graphs.slice_steps(plan):
        assert tuple(sorted(set(steps.tolist()))) == lane_graphs.LENGTHS
    assert plan.max_list_steps == 33                                    # past the 24 prefetched steps of k_iter2
    assert plan.n_tiles > 0 and plan.n_lds_tiles == plan.n_tiles        # every tile in LDS mode ...
    assert max(plan.iter_lds_in, plan.iter_lds_out) <= 1216             # ... and both windows inside the 160 KB
                                                                        # (tests/test_abi_and_host.py: 1216 fits at D = 8)


def _k_iter2_remarks():
    path = os.path.join(REPO, "build", "sell_pipeline.remarks")
    assert os.path.exists(path), "no resource remarks: the library was not built by csrc/Makefile"
    out = {}
    for b in re.split(r"remark: Function Name: ", open(path).read())[1:]:
        name = subprocess.run(["c++filt", b.split()[0]], capture_output=True, text=True).stdout
        m = re.search(r"k_iter2<(\d+), (\d+), (true|false), (true|false), (true|false)>", name)
        if m:
            key = (int(m.group(1)), int(m.group(2))) + tuple(g == "true" for g in m.groups()[2:])
            out[key] = {k: int(re.search(k + r": (\d+)", b).group(1))
                        for k in ("VGPRs", "AGPRs", r"ScratchSize \[bytes/lane\]")}
    return out


def test_every_k_iter2_instantiation_has_zero_scratch():
    kernels = _k_iter2_remarks()
    assert len(kernels) == 27           # 6 shapes x 4 (LAST x XP) + the 3 fused first launches
    for key, res in sorted(kernels.items()):
        assert res[r"ScratchSize \[bytes/lane\]"] == 0, (key, res)
        assert res["AGPRs"] == 0, (key, res)
        assert res["VGPRs"] <= 128, (key, res)                          # 4 waves per SIMD: 1024-thread workgroups


def test_lane_form_is_selected_where_it_was_measured_faster():
    """D = 8, both phases of every launch but the fused first one; -DGNN_QUAD_SWEEP takes it out everywhere."""
    src = open(SOURCE).read()
    sel = re.findall(r"static constexpr bool lane_sweep = ([^;]+);", src)
    assert sel == ["false", "iter2 && D == 8 && !FIRST"], sel
    block = src[src.index("#ifdef GNN_QUAD_SWEEP"):]
    assert block.index("lane_sweep = false") < block.index("#else") < block.index("lane_sweep = iter2") < block.index("#endif")
    # both sweeps of k_iter2 ask Cfg, phase by phase, and nothing else calls the lane form
    assert len(re.findall(r"if constexpr \(Cfg<F, D>::template lane_sweep<FIRST, (?:false|true)>\)\s+sweep16_lane<", src)) == 2
    assert len(re.findall(r"sweep16_lane<", src)) == 2
