"""The graph-convolution classifiers of the reference's toy notebooks on the HIP kernels of csrc/gcn.hip:
GraphConv, GraphConvSelfInt (gnn/GCN_Seg_Toy2D.ipynb cell 20, gnn/GCN_Toy2D.ipynb cell 11), GCNBinaryClassifier
(Seg cell 21, Toy2D cell 13) and GCRNBinaryClassifier (Toy2D cell 14).

Same constructors, sub-module tree and state_dict keys as the notebooks' classes (a reference checkpoint loads);
`forward(x, a)` takes x [B, N, F] and returns logits [B, N]; nn.BCEWithLogitsLoss is applied by the caller.

    h = relu(x Wf^T + bf);  per layer hin = h (GCN) or [h | x] (GCRN)
    GraphConvSelfInt: z = hin Wn^T + bn + (A hin) Wg^T      GraphConv: z = (A hin) Wl^T + bl
    h = relu(z);  out = h Wc^T + bc

The notebooks multiply a dense [B, N, N] adjacency into the features once per layer.  Here the adjacency is
compressed once (`compress_adjacency`) into per-row and per-column lists, and the whole model runs in one launch
forward and two launches backward.  `model(x, adj)` with a SparseAdjacency is the fast form; `model(x, a_dense)`
compresses on every call (two more launches and one host read-back per call) and is the SLOW form.

There is no CPU path: CPU tensors raise RuntimeError, and so does a shape the kernels do not take (the message
names the limit).  No gradient flows to x or a (the notebooks never ask for one): either requiring grad raises.
Parameter gradients flow in training mode (model.train(), grad enabled), as in the notebooks' training_step; in
eval mode the per-layer activations are not kept and the logits carry no graph.

Non-finite values ("Non-finite values in the trainable path"; tests/test_gpu_nonfinite.py): they
propagate, as in torch, by arithmetic alone - no kernel traps and nothing is read back.  The ReLU is torch's:
relu(NaN) = NaN and its derivative passes the gradient wherever h <= 0 does not hold, so a NaN in one weight makes
every logit, the loss and the gradients NaN in the forward and the backward.  A NaN in `x` follows the LISTS: the
nodes reached from the poisoned node within the layers are NaN (forward, and through the column lists backward),
other graphs of the batch keep their bits.  The adjacency keeps its own contract: a status bit, then ValueError
(`compress_adjacency`).
"""
import torch
import torch.nn as nn

from . import _lib


class SparseAdjacency:
    """A [B, N, N] fp32 adjacency as per-row and per-column (transposed) lists, on the device.

    row_cnt [B, N] int32: entries of row i; row_idx / row_val [B, N, W]: their column indices, ascending, and values
    (zero-padded).  col_*: the same for the columns (row indices ascending).  Nothing assumes A is symmetric
    (the notebooks' norm_adjacency is not).  W is ONE width for the whole tensor, so `adj[j:j+32]` is a view -
    which is how the notebooks slice train_A every step.  Built by `compress_adjacency`."""

    def __init__(self, row_cnt, row_idx, row_val, col_cnt, col_idx, col_val):
        self.row_cnt, self.row_idx, self.row_val = row_cnt, row_idx, row_val
        self.col_cnt, self.col_idx, self.col_val = col_cnt, col_idx, col_val

    def __len__(self):
        return int(self.row_cnt.shape[0])

    @property
    def n_nodes(self):
        return int(self.row_cnt.shape[1])

    @property
    def width(self):
        return int(self.row_idx.shape[2])

    @property
    def device(self):
        return self.row_cnt.device

    @property
    def shape(self):
        return (len(self), self.n_nodes, self.n_nodes)

    def __getitem__(self, key):
        if not isinstance(key, slice) or key.step not in (None, 1):
            raise TypeError("SparseAdjacency takes contiguous batch slices, adj[i:j]")
        return SparseAdjacency(self.row_cnt[key], self.row_idx[key], self.row_val[key],
                               self.col_cnt[key], self.col_idx[key], self.col_val[key])

    def to_dense(self, transposed=False):
        """The dense fp32 [B, N, N] tensor, bit for bit what was compressed (a -0.0 entry comes back as +0.0: it
        is not an entry).  `transposed`: rebuilt from the column lists instead (the same tensor)."""
        B, N, W = len(self), self.n_nodes, self.width
        cnt, idx, val = ((self.col_cnt, self.col_idx, self.col_val) if transposed
                         else (self.row_cnt, self.row_idx, self.row_val))
        keep = torch.arange(W, device=self.device).view(1, 1, W) < cnt.unsqueeze(-1)
        dense = torch.zeros((B, N, N), dtype=torch.float32, device=self.device)
        # each slot receives its one entry and zeros from the padding: v + 0 is exact
        dense.scatter_add_(2, idx.long(), torch.where(keep, val, torch.zeros_like(val)))
        return dense.transpose(1, 2).contiguous() if transposed else dense


def compress_adjacency(a):
    """Dense fp32 [B, N, N] on a ROCm device -> SparseAdjacency.  Every entry with a != 0 is kept with its value,
    in ascending index order within each list, so every sum the kernels form has a fixed order.

    Contract for non-finite entries: a NaN or Inf in `a` raises ValueError here.  The dense product of the notebooks
    would spread a NaN to every row (0 * NaN) while a list product would touch only the listed rows, so such an
    adjacency has no faithful compressed form.  The check rides on the ONE host read-back of the compression (the
    list width and a status word); the model's forward and backward read nothing back.

    A NaN in `x` is NOT refused, and here the two products differ as well: torch.matmul(a, x) makes every node of the
    graph NaN, the list product the nodes whose lists reach the poisoned node within the layers.  The kernels keep the
    list semantics: a node the lists reach is NaN, other nodes may stay finite, other graphs keep their bits (module
    docstring, "Non-finite values")."""
    if not torch.is_tensor(a) or not a.is_cuda:
        raise _lib.GnnHipError("compress_adjacency needs a tensor on a ROCm device; there is no CPU path")
    if a.dim() != 3 or a.shape[1] != a.shape[2] or a.dtype != torch.float32:
        raise _lib.GnnHipError("compress_adjacency takes a float32 [B, N, N] tensor, got %s %s"
                               % (a.dtype, tuple(a.shape)))
    if a.requires_grad:
        raise _lib.GnnHipError("the adjacency requires grad: the kernels have no gradient for it")
    rc, ri, rv, cc, ci, cv, _, status = _lib.gcn_compress(a.detach().contiguous())
    if status & 1:
        raise ValueError("the adjacency has a non-finite entry (NaN or Inf): the dense product would spread it to "
                         "every row, the compressed one cannot")
    return SparseAdjacency(rc, ri, rv, cc, ci, cv)


class GraphConv(nn.Module):
    """A (A x) W^T + b (Seg cell 20 / Toy2D cell 11).  A layer of the classifiers below, which run all layers in
    one kernel; it has no forward of its own."""

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.linear = nn.Linear(input_dim, output_dim)

    def forward(self, x, a):
        raise _lib.GnnHipError("GraphConv runs inside GCNBinaryClassifier / GCRNBinaryClassifier (one kernel for "
                               "the whole model); there is no stand-alone or CPU path")


class GraphConvSelfInt(nn.Module):
    """x W1^T + b + (A x) W2^T: a graph convolution with a separate self-interaction term (Seg cell 20 / Toy2D
    cell 11).  A layer of the classifiers below; it has no forward of its own."""

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.node_mod = nn.Linear(input_dim, output_dim)
        self.neighbor_mod = nn.Linear(input_dim, output_dim, bias=False)

    def forward(self, x, a):
        raise _lib.GnnHipError("GraphConvSelfInt runs inside GCNBinaryClassifier / GCRNBinaryClassifier (one kernel "
                               "for the whole model); there is no stand-alone or CPU path")


class GCNBinaryClassifier(nn.Module):
    """Feature extractor, len(hidden_dims) - 1 graph-convolution layers, node classifier head: logits [B, N]
    (Seg cell 21 / Toy2D cell 13)."""
    residual = False

    def __init__(self, input_dim, hidden_dims, gc_type=GraphConvSelfInt):
        super().__init__()
        hidden_dims = [int(d) for d in hidden_dims]
        if not hidden_dims:
            raise ValueError("hidden_dims must name at least the feature extractor's width")
        if not (isinstance(gc_type, type) and issubclass(gc_type, (GraphConv, GraphConvSelfInt))):
            raise TypeError("gc_type must be GraphConv or GraphConvSelfInt")
        self.input_dim, self.hidden_dims = int(input_dim), hidden_dims
        extra = self.input_dim if self.residual else 0
        self.feature_extractor = nn.Linear(self.input_dim, hidden_dims[0])
        self.gc_layers = nn.ModuleList([gc_type(hidden_dims[i] + extra, hidden_dims[i + 1])
                                        for i in range(len(hidden_dims) - 1)])
        self.classifier = nn.Linear(hidden_dims[-1], 1)

    def forward(self, x, a):
        from .autograd import gcn_apply
        return gcn_apply(self, x, a)


class GCRNBinaryClassifier(GCNBinaryClassifier):
    """The same with the input features stacked onto every graph-convolution layer's input, [h | x] (Toy2D
    cell 14)."""
    residual = True
