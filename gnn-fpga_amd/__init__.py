"""MI355X-native SegmentClassifier message-passing hot path (reference gnn/model.py).

Layout: `csrc/` HIP kernels + the C-ABI library (`include/gnn_hip.h`), `_lib.py` the
ctypes binding, `model.py` the drop-in nn.Module tree, `hitgraph.py` the index-form
batch/loader, `synth.py` synthetic inputs, `shard.py` event-batch sharding over ranks,
`graph_build.py` segment graphs from detector hits, `hit_samples.py` the hit classifier's track samples from
detector hits, `muon_graph.py` the muon trigger graphs from EMTF hits, `event_graphs.py` the ACTS full-event graphs
from cluster hits, `select_hits.py` the TrackML barrel hit selection from raw event tables, `metrics.py` confusion
counts, ROC and AUC, `tracks.py` track candidates from scored segments, their matching to particles and their fit, `gcn.py` the toy notebooks' graph-convolution classifiers and their compressed adjacency,
`toy_graphs.py` the toy notebooks' segment and hit graphs built straight into that compressed adjacency,
`cut_study.py` the all-pair histograms and the layer census that choose `build_graphs`' arguments,
`toy_mpnn.py` the toy MPNN notebook's per-iteration segment classifiers and its data cells,
`fixed_point.py` the bit-accurate fixed-point forward of SegmentClassifier and the precision scan over word formats.
"""
from .synth import HitGraph  # noqa: F401
from .hitgraph import HitGraphBatch  # noqa: F401
from .batcher import GraphStore, batch_generator, merge_graphs  # noqa: F401,E402
from .graph_build import build_graphs  # noqa: F401,E402
from .hit_samples import HitSamples, build_hit_samples  # noqa: F401,E402
from .muon_graph import MuonGraphs, build_muon_graphs  # noqa: F401,E402
from .event_graphs import EventGraphs, build_event_graphs  # noqa: F401,E402
from .select_hits import BARREL_VLIDS, SelectedHits, select_hits  # noqa: F401,E402
from .metrics import SegmentMetrics, evaluate  # noqa: F401,E402
from .tracks import Tracks, TrackFit, TrackMatch, build_tracks  # noqa: F401,E402
from .gcn import (GraphConv, GraphConvSelfInt, GCNBinaryClassifier, GCRNBinaryClassifier,  # noqa: F401,E402
                  SparseAdjacency, compress_adjacency)
from .toy_graphs import (ToyHitGraphs, ToySegmentGraphs, build_toy_hit_graphs,  # noqa: F401,E402
                         build_toy_segment_graphs, sort_toy_tracks)
from .cut_study import SegmentCutStudy, count_layer_transitions, study_segment_cuts  # noqa: F401,E402
from .toy_mpnn import (SegmentClassifier as ToySegmentClassifier,  # noqa: F401,E402
                       SegmentClassifier2 as ToySegmentClassifier2, ToyMpnnGraphs, build_toy_mpnn_graphs)
from .fixed_point import (FixedPointFormat, FixedPointScores, FixedPointSegmentClassifier,  # noqa: F401,E402
                          fixed_forward_numpy, quantize_model, scan_precision)
