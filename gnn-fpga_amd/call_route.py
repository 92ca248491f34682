"""Which kernels a SegmentClassifier call runs: decided once per call, here, before the first launch (the rules as two
tables: DESIGN.md section 4, "Which route a model call takes").  `choose_inference` / `choose_training` are pure functions
of plain values; `inference_route` / `training_route` read the knobs off the model, read and bump the per-batch counters
"forwards" / "train_uses" (host entries of `batch.derived`; nobody else does), ask the batch for its event layout, plan and twin at most once and return
a `Route`; its kind stays on the model as `_route.kind` (tests, diagnostics).

  inference  "events"      the whole forward in one launch, one workgroup per graph (k_event)
             "plan"        the fused tile pipeline on the batch's execution plan (csrc/sell_pipeline.hip)
             "per_module"  one kernel per reference module (csrc/gnn_kernels.hip); traces
  training   "events"      one-launch forward and backward (k_event, k_event_bwd)
             "twin"        the batch's level-ordered twin: fused training forward (k_edge_tw), per-pass backward
             "twin_pp"     the twin: per-module training forward, per-pass backward
             "pass"        the caller's batch: per-module training forward, per-pass backward

The per-iteration classifiers of toy_mpnn.py have a rule of their own, `choose_iter` / `iter_route` at the end of this file
("iter_events" or "per_module", inference and training alike), and so has the fixed-point forward of fixed_point.py,
`choose_fixed` ("events" or "per_module").
"""
import collections
import functools
import os

from . import _lib

EVENTS_MAX_GRAPHS = 1024    # one-launch kernels: beyond it the tiled / per-pass kernels fill the chip (tools/latency_probe.py)
TWIN_MIN_HITS = 20000       # smaller batches gain nothing from the level-ordered twin
Choice = collections.namedtuple("Choice", "kind bump")     # bump: the batch's counter (forwards / train_uses) goes up
_EVENTS, _PER_MODULE, _PLAN, _PASS = (Choice(k, False) for k in ("events", "per_module", "plan", "pass"))
# layout: the event layout ("events" only); plan: the execution plan ("plan" only); batch: what the kernels run on
Route = collections.namedtuple("Route", "kind layout plan batch")
# what a model keeps of its last call: the kind alone - the batch, its plan and its twin must not live as long as the
# model does (and the plan's exp-product cache points back at the model: a cycle would hold their memory until a collection)
_KEPT = {k: Route(k, None, None, None) for k in ("events", "plan", "per_module", "twin", "twin_pp", "pass", "iter_events")}


def refuse_unsupported(who, X, F, D, training=False):
    """There is no CPU path and no kernel for other shapes: say so before anything is decided."""
    if not X.is_cuda:
        raise _lib.GnnHipError("%s needs tensors on a ROCm device; there is no CPU path" % who)
    if not _lib.shape_supported(F, D):
        what = "training kernels" if training else "kernel"
        raise _lib.GnnHipError("no HIP %s for input_dim=%d hidden_dim=%d" % (what, F, D))


def first_forward_limit(max_segments, D):
    """`first_forward_max_segments` at width D: up to there a never-seen batch is faster without a plan (tools/
    fresh_probe.py: the crossover is near 6.5 M segments at D <= 16, 3 M at hidden_dim 32, 0.7 M at 64 with T = 6)."""
    return max_segments if D <= 16 else max_segments // 2 if D <= 32 else max_segments * 3 // 20


def choose_inference(F, D, trace, use_events, use_plan, max_segments, n_graphs, n_segments, layout, plan_dim, seen):
    """D: the width the kernels run at; layout: batch.event_layout(); plan_dim: hidden_dim of the plan the batch
    carries (None: no plan); seen: how often the "auto" policy has met this batch ("forwards")."""
    if trace:                                           # every module's output is wanted: full width, no plan
        return _PER_MODULE
    if (use_events and n_graphs <= EVENTS_MAX_GRAPHS and _lib.shape_supported(F, D) and
            _lib.events_preferred(F, D, layout)):
        return _EVENTS
    if not use_plan or not _lib.plan_shape_supported(F, D):
        return _PER_MODULE
    if use_plan != "auto" or plan_dim == D:
        return _PLAN
    # first forward of a never-seen batch: no plan yet - up to the size where the plan pays for itself at once
    fused = seen > 0 or n_segments > first_forward_limit(max_segments, D)
    return Choice("plan" if fused else "per_module", True)


def choose_training(F, D, use_events, policy, n_graphs, n_hits, layout, has_twin, uses, twin_differs=True, fused=True):
    """policy: model.level_order_training; has_twin: the batch has its twin already; uses: its "train_uses";
    twin_differs: batch.level_ordered() is another batch (it returns the batch itself when there is nothing to gain);
    fused: `fused_train_available` of that twin.  The last two are known only once the twin is built: with the
    defaults the answer "twin" means that it is wanted."""
    # (events only when the backward has its one-launch form too: the per-pass backward wants Q_all)
    if use_events and 0 < n_graphs <= EVENTS_MAX_GRAPHS and _lib.events_preferred(F, D, layout, backward=True):
        return _EVENTS
    if not policy or n_hits < TWIN_MIN_HITS:
        return _PASS
    # "auto": the twin (a plan build and two sorts, ten steps' worth) only for a batch object that comes back
    bump = policy == "auto" and not has_twin
    if (bump and uses + 1 < 2) or not twin_differs:
        return Choice("pass", bump)
    return Choice("twin" if fused else "twin_pp", bump)


@functools.lru_cache(maxsize=None)
def _fused_train_shape(F, D):
    """The library's own answer (gnn_plan_route on an empty plan reads the shape only)."""
    return _lib.plan_shape_supported(F, D) and _lib.plan_route(_lib.GnnPlan(), F, D, 0, training=True) is not None


def fused_train_available(twin, F, D):
    """Can the training forward of this plan-space batch (HitGraphBatch.level_ordered) run the fused tile kernels of
    the plan it was made from?  (GNN_NO_FUSED_TRAIN=1 says no: A / B runs.)"""
    plan = twin._fused
    return (plan is not None and twin._fused_dim == D and not os.environ.get("GNN_NO_FUSED_TRAIN") and
            plan.n_pad == twin.n_hits and plan.n_segments == twin.n_segments and _fused_train_shape(F, D))


def inference_route(model, batch, D_run, trace=False):
    """The Route of one inference call of `model` on `batch` at the width `D_run` (_cached_weights)."""
    use_events, n_graphs, plan = model.use_events, batch.n_graphs, batch.plan
    # (the layout is asked for only where it can matter: a batch's first answer costs a pass over its endpoints)
    lay = batch.event_layout() if use_events and not trace and n_graphs <= EVENTS_MAX_GRAPHS else None
    seen = batch.derived("host", "forwards") or 0
    kind, bump = choose_inference(model.input_dim, D_run, trace, use_events, model.use_plan,
                                  model.first_forward_max_segments, n_graphs, batch.n_segments, lay,
                                  None if plan is None else plan.hidden_dim, seen)
    if bump:
        batch.remember("host", "forwards", seen + 1)
    model.__dict__["_route"] = _KEPT[kind]      # (the dict directly: nn.Module.__setattr__ costs more than the decision)
    return Route(kind, lay if kind == "events" else None, batch.build_plan(D_run) if kind == "plan" else None, batch)


def training_route(model, batch):
    """The Route of one training step of `model` on `batch` (autograd and GradBucket.step alike)."""
    F, D = model.input_dim, model.hidden_dim
    use_events = getattr(model, "use_events", True)
    lay = batch.event_layout() if use_events and 0 < batch.n_graphs <= EVENTS_MAX_GRAPHS else None
    uses = batch.derived("host", "train_uses") or 0
    facts = (F, D, use_events, getattr(model, "level_order_training", "auto"), batch.n_graphs, batch.n_hits, lay,
             batch.derived("features", "twin") is not None, uses)
    c, run = choose_training(*facts), batch
    if c.kind == "twin":                        # wanted: build it (once per batch) and ask again with what came out
        twin = batch.level_ordered(D)
        c = choose_training(*facts, twin_differs=twin is not batch, fused=fused_train_available(twin, F, D))
        run = batch if c.kind == "pass" else twin
    if c.bump:
        batch.remember("host", "train_uses", uses + 1)
    model.__dict__["_route"] = _KEPT[c.kind]
    return Route(c.kind, lay if c.kind == "events" else None, None, run)


# ---- the per-iteration classifiers of toy_mpnn.py (gnn/MPNN_Seg_Toy2D.ipynb cell 14) ------------------------------------
def choose_iter(use_events, n_graphs, layout, n_iters, fits):
    """The route of one toy_mpnn call, inference and training alike: "iter_events" - the whole forward (and backward)
    in one launch, one workgroup per graph, a weight set per pass (csrc/iter_events.hip) - or "per_module", the
    notebook's forward module by module on the per-module kernels, which takes every shape and size.
    layout: batch.event_layout() (None: not block-diagonal, or a graph beyond _lib.EVENTS_MAX_SEGMENTS); fits:
    gnn_iter_events_supported for the largest graph (with the backward when the call trains)."""
    if use_events and 0 < n_graphs <= EVENTS_MAX_GRAPHS and layout is not None and n_iters <= _lib.GNN_ITER_MAX and fits:
        return "iter_events"
    return "per_module"


def iter_route(model, batch, training):
    """The Route of one call of a toy_mpnn model on `batch`; its kind stays on the model as `_route.kind`."""
    use_events = model.use_events
    lay = batch.event_layout() if use_events and 0 < batch.n_graphs <= EVENTS_MAX_GRAPHS else None
    fits = lay is not None and _lib.iter_events_supported(model.input_dim, model.hidden_dim, lay.max_hits,
                                                          lay.max_segments, training)
    kind = choose_iter(use_events, batch.n_graphs, lay, model.n_iters, fits)
    model.__dict__["_route"] = _KEPT[kind]
    return Route(kind, lay if kind == "iter_events" else None, None, batch)


# ---- the fixed-point forward of fixed_point.py (include/gnn_hip_fixed.h, include/gnn_hip_fixed_events.h) ------------------
def choose_fixed(use_events, trace, n_graphs, layout, fits):
    """The route of one FixedPointSegmentClassifier call: "events" - the whole forward in one launch, one workgroup per
    graph (csrc/fixed_events.hip), which also counts the overflows of every graph - or "per_module", one kernel per
    reference module (csrc/fixed_point.hip), which takes every size and keeps the traces.  Both give the same bits.
    layout: batch.event_layout(); fits: gnn_fxev_supported for the largest graph at the format's table_bits."""
    if use_events and not trace and 0 < n_graphs <= EVENTS_MAX_GRAPHS and layout is not None and fits:
        return "events"
    return "per_module"
