"""NaN and Inf cases for the trainable path (test infrastructure, not a test module; shared by test_nonfinite_host.py
and test_gpu_nonfinite.py): SegmentClassifier on every route, NodeClassifier, the graph-convolution classifiers and the
fused BCELoss.  The contract they hold is written down in INTEGRATION.md ("Non-finite values").

  the poisons   NaN with four bit patterns (quiet, the smallest signalling payload, all mantissa bits, all bits), +-inf
  the batches   `seg_batch`: the route recorders' two graphs (tools/record_backward_routes.py: 900 hits / 6000 segments
                and 9 hits / 11 segments) between two more copies of the small one - the recorders' own batch has two
                graphs and therefore no middle one - every 13th segment padded (src = dst = -1), hits without
                segments: 927 hits, 6033 segments.  `muon_batch`: the 8 synth.muon_graph events of
                test_gpu_call_route.py.  `twin_batch`: that file's 21 000 hits, the smallest the level-ordered twin
                takes.  The poison always sits in a MIDDLE graph: oracle.index_torch gathers row 0 for a padded
                segment and multiplies it by zero, so a NaN in hit 0 would make every padded score NaN there and
                nowhere else (index_c, nodeclf_fp64 and the kernels read no hit for a padded segment)
  the sites     `x_sites`: first hit, last hit, a hit without segments, and - given a plan - the first hit of a tile
                (a tile and window boundary) of the poisoned graph; `w_site`: the middle element of each weight
  the truth     `scores64` / `scores_c`: oracle.index_torch and oracle.index_c; `expected_mask`: the NaN mask a kernel
                must show - index_torch's in fp64 on the valid segments, index_c's on the padded ones (see above; the
                host test holds the oracles to each other on everything else); `bce_terms`: the BCE reference;
                `train_reference`: loss and the ten gradients through it; `gcn_list_run`: tests/gcn_fp64.py's model
                with A hin as a sum over the non-zero entries of A in index order - the kernels' list semantics
"""
import copy
import functools

import numpy as np
import torch
import torch.nn as nn

import gcn_fp64
import nodeclf_fp64
from oracle import index_c, index_torch
from oracle.dense_torch import KEYS

NAN_BITS = {"quiet": 0x7FC00000, "payload1": 0x7F800001, "allmantissa": 0x7FFFFFFF, "allbits": 0xFFFFFFFF}
INFS = {"+inf": float("inf"), "-inf": float("-inf")}


def f32(bits):
    """The float32 with this bit pattern (numpy scalar: assigning it into a float32 array keeps the payload)."""
    return np.array([bits], np.uint32).view(np.float32)[0]


NANS = {k: f32(v) for k, v in NAN_BITS.items()}
QNAN = NANS["quiet"]


def put(t, flat_index, value):
    """`t` (float32 tensor) with one element replaced, bit for bit (a NaN's payload survives: the copy is by bits)."""
    a = t.detach().cpu().numpy().copy()
    a.reshape(-1).view(np.uint32)[flat_index] = np.array([value], np.float32).view(np.uint32)[0]
    return torch.from_numpy(a)


# ---- batches --------------------------------------------------------------------------------------------------------
def _padded(b):
    from gnn_fpga_amd import HitGraphBatch
    src, dst = b.src.numpy().copy(), b.dst.numpy().copy()
    src[7::13] = -1
    dst[7::13] = -1
    return HitGraphBatch(b.X.numpy(), src, dst, hit_ptr=b.hit_ptr, seg_ptr=b.seg_ptr)


@functools.lru_cache(maxsize=None)
def seg_batch(F=3):
    from gnn_fpga_amd import HitGraphBatch, synth
    small = lambda seed: synth.layered_graph(9, 11, F, n_layers=3, seed=seed)       # noqa: E731
    graphs = [small(72), synth.layered_graph(900, 6000, F, seed=70), small(71), small(73)]
    return _padded(HitGraphBatch.from_graphs(graphs))


SEG_GRAPH = 1           # the poisoned graph of seg_batch: the 900-hit one, with small graphs on either side


@functools.lru_cache(maxsize=None)
def muon_batch():
    from gnn_fpga_amd import HitGraphBatch, synth
    return HitGraphBatch.from_graphs([synth.muon_graph(s) for s in range(8)])


MUON_GRAPH = 4


@functools.lru_cache(maxsize=None)
def twin_batch():
    from gnn_fpga_amd import HitGraphBatch, synth
    return HitGraphBatch.from_graphs([synth.layered_graph(7000, 40000, 3, seed=10 + s) for s in range(3)])


TWIN_GRAPH = 1


def with_X(b, X):
    """The host batch `b` with other features (a new object: nothing derived is shared)."""
    from gnn_fpga_amd import HitGraphBatch
    return HitGraphBatch(np.asarray(X, np.float32), b.src.numpy(), b.dst.numpy(), hit_ptr=b.hit_ptr, seg_ptr=b.seg_ptr)


def poisoned_X(b, hit, value, feature=0):
    X = b.X.numpy().copy()
    X.view(np.uint32)[hit, feature] = np.array([value], np.float32).view(np.uint32)[0]
    return X


def segments_of_graphs(b, graphs):
    """bool [E]: the segments of these graphs."""
    m = np.zeros(b.n_segments, bool)
    for g in graphs:
        m[int(b.seg_ptr[g]):int(b.seg_ptr[g + 1])] = True
    return m


# ---- sites ----------------------------------------------------------------------------------------------------------
def x_sites(b, graph, plan=None):
    """{name: hit} in `graph` of the host batch `b`.  "lonely": the first hit no valid segment touches, in this graph
    or else in another middle graph of the batch (seg_batch: in the small graph after the poisoned one; absent where
    no middle graph has one); "tile": with `plan` (the batch's execution plan, any builder's), the hit in the
    first slot of the last tile that starts inside the graph - a tile boundary and, with it, a window boundary."""
    lo, hi = int(b.hit_ptr[graph]), int(b.hit_ptr[graph + 1])
    src, dst = b.src.numpy(), b.dst.numpy()
    deg = np.bincount(np.concatenate([src[src >= 0], dst[dst >= 0]]), minlength=b.n_hits)
    out = {"first": lo, "last": hi - 1}
    for g in [graph] + [k for k in range(1, b.n_graphs - 1) if k != graph]:
        glo, ghi = int(b.hit_ptr[g]), int(b.hit_ptr[g + 1])
        lonely = np.flatnonzero(deg[glo:ghi] == 0)
        if lonely.size:
            out["lonely"] = glo + int(lonely[0])
            break
    if plan is not None:
        perm = plan.perm.cpu().numpy()
        starts = plan.tiles.cpu().numpy().reshape(-1, 8)[:, 0].astype(np.int64) * 16
        heads = perm[starts[starts > 0]]
        heads = heads[(heads >= lo) & (heads < hi)]
        assert heads.size, "no tile starts inside the poisoned graph"
        out["tile"] = int(heads[-1])
    return out


def w_site(w):
    """The flat index of the poisoned element of a weight tensor: the middle one."""
    return int(w.numel()) // 2


# ---- the segment classifier's oracles ----------------------------------------------------------------------------------
def _params(weights, dtype):
    return {k: torch.as_tensor(np.asarray(w)).to(dtype) for k, w in zip(KEYS, weights)}


def scores64(X, b, weights, T, dtype=torch.float64):
    """oracle.index_torch's scores [E] as a float64 array, computed in `dtype`."""
    with torch.no_grad():
        e = index_torch.segment_classifier(np.asarray(X), b.src.numpy().astype(np.int64), b.dst.numpy().astype(np.int64),
                                           _params(weights, dtype), T)
    return e.double().numpy()


def scores_c(X, b, weights, T, f64=True):
    p = {k: np.asarray(w, np.float32) for k, w in zip(KEYS, weights)}
    return index_c.segment_classifier(np.asarray(X, np.float32), b.src.numpy(), b.dst.numpy(), p, T, f64=f64)


def expected_mask(X, b, weights, T):
    """(NaN mask [E] a kernel must show, fp64 scores): index_torch's mask on the valid segments, index_c's on the
    padded ones."""
    e = scores64(X, b, weights, T)
    mask = np.isnan(e)
    pad = b.src.numpy() < 0
    if pad.any():
        mask[pad] = np.isnan(scores_c(X, b, weights, T))[pad]
    return mask, e


# ---- BCE ------------------------------------------------------------------------------------------------------------
def bce_terms(e, y):
    """torch.nn.BCELoss's terms [n] without its range check, in the dtype of `e` (float64 for a reference):
    -(y clamp(log e, min=-100) + (1 - y) clamp(log1p(-e), min=-100)).  NaN for a score that is NaN or outside [0, 1]
    and for a NaN label."""
    return -(y * torch.clamp(torch.log(e), min=-100.0) + (1.0 - y) * torch.clamp(torch.log1p(-e), min=-100.0))


def bce_grad(e, y):
    """The gradient of sum(bce_terms) the kernels are held to: NaN wherever the term is NaN, torch.nn.BCELoss's own
    backward (e - y) / max(e (1 - e), 1e-12) elsewhere.  (Autograd through bce_terms is that formula inside (0, 1);
    it is NOT NaN at a score outside [0, 1] - clamp's backward gives 0 for a NaN input - and it IS NaN at exactly 0
    and 1, where 0 * inf appears: test_nonfinite_host.py shows all three.)"""
    g = (e - y) / torch.clamp(e * (1.0 - e), min=1e-12)
    return torch.where(torch.isnan(bce_terms(e, y)), torch.full_like(g, float("nan")), g)


def labels(n, seed=0):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.4).float()


def train_reference(X, b, weights, T, y, dtype=torch.float64):
    """(loss, [ten gradients as float64 arrays]) of mean(bce_terms(scores, y)) through oracle.index_torch."""
    p = {k: v.clone().requires_grad_(True) for k, v in _params(weights, dtype).items()}
    e = index_torch.segment_classifier(np.asarray(X), b.src.numpy().astype(np.int64), b.dst.numpy().astype(np.int64), p, T)
    loss = bce_terms(e, y.to(dtype)).mean()
    loss.backward()
    return float(loss.detach()), [p[k].grad.double().numpy() for k in KEYS]


# ---- NodeClassifier -------------------------------------------------------------------------------------------------
def nodeclf_reference(X, b, weights12, T, y=None, dtype=torch.float64):
    """(hit scores [N] float64, loss, [twelve gradients]) of tests/nodeclf_fp64.py's model; loss and gradients (of
    mean(bce_terms(scores, y))) only with labels."""
    w = [torch.as_tensor(np.asarray(t)).to(dtype).clone().requires_grad_(y is not None) for t in weights12]
    s, _ = nodeclf_fp64._forward(torch.as_tensor(np.asarray(X)).to(dtype), b.src.long(), b.dst.long(), w, T)
    if y is None:
        return s.detach().double().numpy(), None, None
    loss = bce_terms(s, y.to(dtype)).mean()
    loss.backward()
    return s.detach().double().numpy(), float(loss.detach()), [t.grad.double().numpy() for t in w]


# ---- graph-convolution classifiers ----------------------------------------------------------------------------------
class ListGCN(nn.Module):
    """A gcn_fp64.DenseGCN whose A hin is the LIST product: a sum over the non-zero entries of A, in index order.  A
    zero entry is no entry: 0 * NaN does not arise, and a NaN in one node's features reaches the nodes that list it -
    not, as in torch.matmul(a, x), every node of the graph."""

    def __init__(self, dense):
        super().__init__()
        self.m = dense

    def forward(self, x, a, keep=None):
        m = self.m
        B, N, _ = a.shape
        nz = a.nonzero()                                        # lexicographic: batch, row, column
        vals = a[nz[:, 0], nz[:, 1], nz[:, 2]][:, None]
        rows, cols = nz[:, 0] * N + nz[:, 1], nz[:, 0] * N + nz[:, 2]
        h = torch.relu(m.feature_extractor(x))
        if keep is not None:
            keep.append(h)
        for layer in m.gc_layers:
            hin = torch.cat([h, x], dim=-1) if m.residual else h
            flat = hin.reshape(B * N, -1)
            ah = flat.new_zeros(flat.shape).index_add(0, rows, vals * flat[cols]).reshape(hin.shape)
            z = layer.node_mod(hin) + layer.neighbor_mod(ah) if m.conv == "selfint" else layer.linear(ah)
            h = torch.relu(z)
            if keep is not None:
                keep.append(h)
        return m.classifier(h).squeeze(-1)


def gcn_list_run(model, x, a, y=None, dtype=torch.float64):
    """gcn_fp64.run with the list product: logits, per-layer h and - with labels - loss and gradients (named as the
    dense model's parameters are)."""
    res = gcn_fp64.run(ListGCN(copy.deepcopy(model)), x, a, y, dtype)
    if "grads" in res:
        res["grads"] = {k[len("m."):]: v for k, v in res["grads"].items()}
    return res


def gcn_reach(a, graph, node, layers):
    """bool [N]: the nodes of `graph` the list form reaches from `node` within `layers` products (a row i lists j
    where A[i, j] != 0), the node itself included."""
    nzt = (np.asarray(a[graph]) != 0)
    reach = np.zeros(nzt.shape[0], bool)
    reach[node] = True
    for _ in range(layers):
        reach = reach | (nzt[:, reach].any(axis=1))
    return reach
