"""Histogram-based tree grower (the `hist` / `gpu_hist` updater).

Replaces xgboost's grow_quantile_histmaker / updater_gpu_hist (the native
hot loop behind xgb.train). The design is level-synchronous and
segment-based — all per-level device work is batched so a level costs a
fixed small number of kernel launches and exactly ONE device→host sync (the
partition left-counts readback):

  1. histogram build for the new frontier — only the smaller child (by
     global hessian) of each sibling pair is built; the larger is derived by
     the subtraction trick from the cached parent histogram;
  2. (distributed) ONE fused allreduce of the level's histogram accumulator
     across ranks over RCCL/xGMI (int64 fixed-point on GPU: the sum is
     bit-deterministic and rank-order independent);
  3. batched split-gain scan over all (feature, bin) candidates including
     both missing directions;
  4. batched partition of all split nodes' row segments into the
     opposite-parity row buffer (two-ended compaction in the same range).

Row sets live in two ping-pong int32 buffers; a node's segment is
(parity, start, end) and children occupy the parent's range in the other
buffer, so leaves finalized at different depths coexist without copies.

Backend ops come from ops.backend_for(device): CDNA4 HIP kernels on MI355X,
torch reference on CPU.
"""
import heapq
import logging
import os

import numpy as np
import torch

from .. import ops
from .tree import Tree, cat_members

logger = logging.getLogger(__name__)


class GrowParams:
    def __init__(self, params):
        p = params or {}
        self.eta = float(p.get("eta", p.get("learning_rate", 0.3)))
        self.max_depth = int(p.get("max_depth", 6))
        self.max_leaves = int(p.get("max_leaves", 0))
        self.grow_policy = p.get("grow_policy", "depthwise")
        self.reg_lambda = float(p.get("lambda", p.get("reg_lambda", 1.0)))
        self.reg_alpha = float(p.get("alpha", p.get("reg_alpha", 0.0)))
        self.gamma = float(p.get("gamma", p.get("min_split_loss", 0.0)))
        self.min_child_weight = float(p.get("min_child_weight", 1.0))
        self.max_delta_step = float(p.get("max_delta_step", 0.0))
        self.subsample = float(p.get("subsample", 1.0))
        self.sampling_method = str(p.get("sampling_method") or "uniform")
        if self.sampling_method not in ("uniform", "gradient_based"):
            raise ValueError(
                "sampling_method must be 'uniform' or 'gradient_based', got %r" % self.sampling_method
            )
        self.colsample_bytree = float(p.get("colsample_bytree", 1.0))
        self.colsample_bylevel = float(p.get("colsample_bylevel", 1.0))
        self.colsample_bynode = float(p.get("colsample_bynode", 1.0))
        # xgboost accepts the SageMaker string forms "(1,-1,0)" and
        # "[[0,1],[2,3]]" directly (the reference forwards hyperparameter
        # strings as-is) — normalize them here so trainer.train keeps that
        # surface
        mc = p.get("monotone_constraints")
        if isinstance(mc, str):
            body = mc.strip().strip("()[]")
            mc = tuple(int(float(t)) for t in body.split(",") if t.strip()) if body else None
        self.monotone_constraints = mc
        ic = p.get("interaction_constraints")
        if isinstance(ic, str):
            import ast

            ic = ast.literal_eval(ic) if ic.strip() else None
        self.interaction_constraints = ic
        # categorical split search: a feature with fewer categories than
        # max_cat_to_onehot tries one category against the rest, the others
        # a sorted partition whose smaller side holds at most
        # max_cat_threshold categories
        self.max_cat_to_onehot = int(p.get("max_cat_to_onehot", 4))
        self.max_cat_threshold = int(p.get("max_cat_threshold", 64))
        # Accepted for xgboost parity; this framework is ALWAYS deterministic.
        # A float-atomic LDS fast path for "false" was built and measured
        # 3x SLOWER than the int64 fixed-point slab (80.9 vs 239.4 r/s on the
        # 12.5M-row bench — ds_add_f32 throughput; see
        # profiles/r01_optimization_log.md), so the flag costs nothing here.
        self.deterministic_histogram = str(
            p.get("deterministic_histogram", "true")
        ).lower() not in ("false", "0")
        if self.max_depth == 0 and self.max_leaves == 0 and self.grow_policy == "depthwise":
            self.max_depth = 6


class _Node:
    __slots__ = ("nid", "parity", "start", "end", "g", "h", "depth", "lower", "upper", "allowed", "sum32")

    def __init__(self, nid, parity, start, end, g, h, depth, lower=-float("inf"), upper=float("inf"), allowed=None,
                 sum32=None):
        self.nid = nid
        self.parity = parity
        self.start = start
        self.end = end
        self.g = g
        self.h = h
        self.depth = depth
        self.lower = lower   # monotone-constraint weight bounds
        self.upper = upper
        self.allowed = allowed  # interaction-constraint feature mask (f,) bool or None
        # (G, H) in the device grower's float32 arithmetic (a right child's
        # by float32 subtraction from its parent's, as make_level derives
        # them); None where the per-level loop does not mirror that grower
        self.sum32 = sum32

    @property
    def seg(self):
        return (self.start, self.end)


class HistGrower:
    def __init__(self, qm, params, comm=None, generator=None):
        self.qm = qm
        self.p = GrowParams(params)
        self.comm = comm  # optional: allreduce_(tensor) / allreduce_max_(tensor) / rank
        self.backend = ops.backend_for_qm(qm)
        self.device = qm.device
        self.generator = generator
        self.state = None
        f = qm.num_col
        self.monotone = None
        self._monotone_host = None  # the same vector as host ints
        if self.p.monotone_constraints:
            mono = list(self.p.monotone_constraints)[:f] + [0] * max(0, f - len(self.p.monotone_constraints))
            if any(mono):
                self.monotone = torch.tensor(mono, dtype=torch.int8, device=self.device)
                self._monotone_host = [int(c) for c in mono]
        # categorical columns (host bools; None without one): their splits
        # are category sets, searched and partitioned by the per-level path
        is_cat = getattr(qm, "is_cat", None)
        self._is_cat_host = [bool(c) for c in is_cat.tolist()] if is_cat is not None else None
        self._split_kwargs = {}
        if self._is_cat_host is not None:
            self._split_kwargs = {
                "max_cat_to_onehot": self.p.max_cat_to_onehot,
                "max_cat_threshold": self.p.max_cat_threshold,
            }
            if self._monotone_host is not None:
                for j, (c, m) in enumerate(zip(self._is_cat_host, self._monotone_host)):
                    if c and m:
                        raise ValueError(
                            f"monotone constraint on categorical feature {j}: a category set "
                            "has no order to constrain"
                        )
        # "device" or "per_level": which grower path the last tree took
        self.grow_path = None
        # On a backend that declares MIRRORS_DEVICE_GROWER (the HIP backends:
        # dense, which has the device grower, and sparse, which grows per
        # level only) the per-level depthwise loop reproduces the device
        # grower's arithmetic, so every device path grows the same trees:
        # the root (G, H) rounded to float32 before leaf weights subtract
        # from it (the device reads node_gh[0] back), and float32 node sums
        # into the split scan. Elsewhere it keeps float64 sums.
        self._mirror_device = (
            bool(getattr(self.backend, "MIRRORS_DEVICE_GROWER", False))
            and self.p.grow_policy != "lossguide"
        )
        self._fallback_logged = False
        self._sampling_logged = False
        self.inter_sets = None
        if self.p.interaction_constraints:
            self.inter_sets = [set(group) for group in self.p.interaction_constraints]

    # -- weight / gain math (host scalars; double precision) ---------------
    def _weight(self, g, h, lower=-float("inf"), upper=float("inf")):
        a = abs(g) - self.p.reg_alpha
        if a < 0:
            a = 0.0
        w = -(a if g > 0 else -a) / (h + self.p.reg_lambda)
        if self.p.max_delta_step > 0:
            w = max(-self.p.max_delta_step, min(self.p.max_delta_step, w))
        return max(lower, min(upper, w))

    def _interaction_allowed(self, parent_allowed, feature):
        """Child feature mask after splitting on `feature` (xgboost rule:
        child candidates = parent candidates ∩ (∪ sets containing feature,
        plus the feature itself))."""
        if self.inter_sets is None:
            return None
        f = self.qm.num_col
        allowed = torch.zeros(f, dtype=torch.bool, device=self.device)
        allowed[feature] = True
        for group in self.inter_sets:
            if feature in group:
                for idx in group:
                    if idx < f:
                        allowed[idx] = True
        if parent_allowed is not None:
            allowed &= parent_allowed
        return allowed

    def _node_mask(self, base_mask, node):
        if node.allowed is None:
            return base_mask
        if base_mask is None:
            return node.allowed
        return base_mask & node.allowed

    @staticmethod
    def _sample_count(frac, avail_count):
        """How many of `avail_count` features a colsample draw keeps."""
        if frac >= 1.0:
            return avail_count
        return max(1, int(round(frac * avail_count)))

    def _sample_features(self, frac, prev_mask, prev_count=None):
        """Draw a feature mask of `frac` of the features set in `prev_mask`
        (all features when None). `prev_count`, the number of features set
        in `prev_mask` when the caller knows it, selects them without the
        host sync of nonzero(); the draw is the same either way."""
        f = self.qm.num_col
        if frac >= 1.0:
            return prev_mask
        if prev_mask is None:
            avail = torch.arange(f, device=self.device)
        elif prev_count is None:
            avail = prev_mask.nonzero().flatten()
        else:
            # stable sort of the inverted mask lists the set positions
            # first, in ascending order: nonzero() with a known length
            avail = torch.sort((~prev_mask).to(torch.uint8), stable=True).indices[:prev_count]
        k = max(1, int(round(frac * avail.numel())))
        perm = torch.randperm(avail.numel(), device=self.device, generator=self.generator)[:k]
        mask = torch.zeros(f, dtype=torch.bool, device=self.device)
        mask[avail[perm]] = True
        return mask

    def _allreduce(self, tensor):
        if self.comm is not None:
            self.comm.allreduce_(tensor)
        return tensor

    def _build_level_hists(self, gh, scale, build_nodes, derived, node_hist):
        """build_nodes: [_Node] (all same parity); derived: [(nid, parent, sib)]."""
        if build_nodes:
            acc = self.state.build_histograms(
                [n.seg for n in build_nodes], build_nodes[0].parity, scale
            )
            self._allreduce(acc)
            hist = self.backend.hist_to_float(acc, scale)
            for i, node in enumerate(build_nodes):
                node_hist[node.nid] = hist[i]
        for nid, parent_nid, sibling_nid in derived:
            node_hist[nid] = node_hist[parent_nid] - node_hist[sibling_nid]

    def _sample_rows(self, gh):
        """This tree's row sample: (rows, gh_for_tree). `rows` is an
        ascending int32 row list, or None for the full data (level 0 then
        streams the original matrix).

        uniform keeps each row with probability `subsample`.
        gradient_based (Minimal Variance Sampling) keeps row i with
        probability p_i = min(1, r_i / mu), r_i = sqrt(g_i^2 + h_i^2), where
        sum_i p_i = subsample * n, and multiplies a kept pair by 1 / p_i:
        gh_for_tree is that rescaled tensor. Both draw one rand(n) from the
        same generator at the same place. With a communicator every rank
        thresholds its own shard (no collective).
        """
        p = self.p
        if p.subsample >= 1.0:
            return None, gh
        n = self.qm.num_row
        u = torch.rand(n, device=self.device, generator=self.generator)
        if p.sampling_method != "gradient_based":
            return (u < p.subsample).nonzero(as_tuple=True)[0].to(torch.int32), gh
        if not self._sampling_logged:
            self._sampling_logged = True
            logger.info(
                "sampling_method=gradient_based: each tree samples about %.3g of the rows by "
                "gradient magnitude%s",
                p.subsample,
                " (threshold computed per rank, on its own shard)" if self.comm is not None else "",
            )
        return self.backend.gradient_sample(gh, p.subsample, u)

    def _gradient_sampled(self, sample_rows):
        """Does this tree draw a gradient-based sample? Such a tree's leaf
        values belong on every training row's margin: the rows it dropped
        are the well-fitted ones, not a random subset."""
        return (
            sample_rows is None
            and self.p.subsample < 1.0
            and self.p.sampling_method == "gradient_based"
        )

    def grow(self, gh, sample_rows=None):
        """Grow one tree from (n, 2) float32 gradients.

        Returns (tree, leaf_jobs) where leaf_jobs is a list of
        (parity, start, end, leaf_value) covering this rank's rows; pass to
        backend.update_margins together with self.bufs.
        """
        qm = self.qm
        p = self.p
        if sample_rows is not None:
            rows = sample_rows
        else:
            rows, gh = self._sample_rows(gh)

        self.state = self.backend.make_tree_state(qm, gh, rows)
        self.state.margin_all_rows = self._gradient_sampled(sample_rows)
        self.tree_rows = rows  # the rows this tree grows on (None: all)
        cap = self.state.cap

        scale = self.backend.compute_scale(gh, comm=self.comm)
        tree_mask = self._sample_features(p.colsample_bytree, None)

        # device-autonomous fast path: the whole depthwise tree enqueued
        # with zero host syncs (one readback at the end)
        if self._device_grow_ok():
            self.grow_path = "device"
            tree, leaf_jobs = self._grow_depthwise_device(gh, scale, cap, tree_mask)
            tree.finalize()
            return tree, leaf_jobs

        self.grow_path = "per_level"
        tree = Tree()
        cached = getattr(gh, "_smxgb_rootsum", None) if rows is None else None
        root_sum = (
            cached.clone()
            if cached is not None
            else (
                gh.to(torch.float64).sum(0)
                if rows is None
                else gh.index_select(0, rows.long()).to(torch.float64).sum(0)
            )
        )
        root_sum = self._allreduce(root_sum)
        G, H = float(root_sum[0]), float(root_sum[1])
        sum32 = None
        if self._mirror_device:
            sum32 = (np.float32(G), np.float32(H))
            G, H = float(sum32[0]), float(sum32[1])
        root = tree.add_node(parent=-1, value=self._weight(G, H) * p.eta, sum_hess=H)
        root_node = _Node(root, 0, 0, cap, G, H, 0, sum32=sum32)

        if p.grow_policy == "lossguide":
            leaf_jobs = self._grow_lossguide(tree, gh, scale, root_node, tree_mask)
        else:
            leaf_jobs = self._grow_depthwise(tree, gh, scale, root_node, tree_mask)
        tree.finalize()
        return tree, leaf_jobs

    def _constrained(self):
        """Any hyperparameter that needs per-level or per-node candidate
        state (monotone / interaction constraints, level or node colsample)."""
        p = self.p
        return (
            self.monotone is not None
            or self.inter_sets is not None
            or p.colsample_bylevel < 1.0
            or p.colsample_bynode < 1.0
        )

    def _device_fallback_reason(self):
        """Why this configuration cannot use the device grower (None when
        it can)."""
        p = self.p
        if self._is_cat_host is not None:
            return "categorical features"
        if p.grow_policy != "depthwise":
            return "grow_policy=%s (lossguide)" % p.grow_policy
        if p.max_leaves != 0:
            return "max_leaves=%d" % p.max_leaves
        if p.max_depth > 10:
            return "max_depth=%d above 10" % p.max_depth
        if p.max_depth < 1:
            return "max_depth=%d" % p.max_depth
        if self.comm is not None and self._constrained():
            return "monotone/interaction constraints or level/node colsample with a communicator"
        return None

    def _device_grow_ok(self):
        if not hasattr(self.backend, "DeviceGrower") or os.environ.get("SMXGB_NO_DEVICE_GROW") == "1":
            return False
        reason = self._device_fallback_reason()
        if reason is not None and not self._fallback_logged:
            self._fallback_logged = True
            logger.debug("device grower not used, growing per level: %s", reason)
        return reason is None

    def _device_grower_for(self, slot):
        """One DeviceGrower (own heap buffers) per (depth, matrix, slot)."""
        key = (self.p.max_depth, id(self.qm), slot)
        growers = getattr(self, "_device_growers", None)
        if growers is None:
            growers = {}
            self._device_growers = growers
        dg = growers.get(key)
        if dg is None:
            dg = self.backend.DeviceGrower(
                self.state, self.p.max_depth,
                monotone=self.monotone, interaction_sets=self.inter_sets,
            )
            growers[key] = dg
        return dg

    def _grow_depthwise_device(self, gh, scale, cap, tree_mask):
        """Consume the DeviceGrower's one-readback result into a Tree."""
        p = self.p
        dg = self._device_grower_for(0)
        dg.state = self.state  # fresh per-tree compact state
        dg.traverse = self._traverse_ok(self.state)
        level_states = None
        if p.colsample_bylevel < 1.0 or p.colsample_bynode < 1.0:
            level_masks, level_states = self._draw_level_masks(tree_mask)
            dg.mask = level_masks
        elif tree_mask is not None:
            dg.mask = tree_mask.to(torch.uint8).contiguous()
        splits_np, counts_np, root_np = dg.grow(
            scale, (p.reg_lambda, p.reg_alpha, p.gamma, p.min_child_weight), self.comm
        )
        self.state._level0 = not bool(splits_np[0, 0] > 0)
        tree, leaf_jobs = self._build_tree_from_heap(splits_np, counts_np, root_np, cap)
        self._bind_traverse(self.state, dg)
        if level_states is not None and self._live_levels < p.max_depth:
            # the per-level loop stops drawing once the frontier is empty:
            # leave the generator where its last live level's draws did
            self._rng().set_state(level_states[self._live_levels - 1])
        return tree, leaf_jobs

    @staticmethod
    def _traverse_ok(state):
        """This tree's margins can be updated by traversal (the hip compact
        state on the full-data path); decided before the tree is enqueued
        because it also drops the deepest level's partition."""
        ok = getattr(state, "traverse_ok", None)
        return bool(ok()) if ok is not None else False

    def _bind_traverse(self, state, dg):
        """Hand the state what update_margins needs to traverse: the
        grower's device split heap (valid until its next enqueue) and the
        heap index of every leaf_jobs entry, in order — the caller may
        rescale the values (DART) but keeps the order."""
        if dg.traverse:
            state._traverse = (dg.splits, self.p.max_depth, self._leaf_heap)

    def _rng(self):
        if self.generator is not None:
            return self.generator
        if self.device.type == "cuda":
            index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            return torch.cuda.default_generators[index]
        return torch.default_generator

    def _draw_level_masks(self, tree_mask):
        """Pre-draw the colsample_bylevel / colsample_bynode masks of all
        max_depth levels in the per-level loop's order (level draw, then the
        node draw from it), with no host sync. Returns the uint8 [D, f]
        table (tree mask folded in) and the generator state after each
        level. A tree that stops early rewinds to the state after its last
        live level, which is where drawing only that many levels ends."""
        p = self.p
        f = self.qm.num_col
        gen = self._rng()
        tree_count = self._sample_count(p.colsample_bytree, f)
        level_count = self._sample_count(p.colsample_bylevel, tree_count)
        rows, states = [], []
        for _ in range(p.max_depth):
            level_mask = self._sample_features(p.colsample_bylevel, tree_mask, tree_count)
            node_mask = self._sample_features(p.colsample_bynode, level_mask, level_count)
            rows.append(node_mask)
            states.append(gen.get_state())
        return torch.stack(rows).to(torch.uint8).contiguous(), states

    def device_async_ok(self):
        """True when a round's independent trees (multiclass / bagging) can
        be enqueued back-to-back via grow_async/grow_finish."""
        p = self.p
        # level / node colsample stay sequential: several in-flight trees
        # sharing one generator cannot reproduce the sequential draw order
        # (each tree's rewind depends on its own readback)
        return (
            self.comm is None
            and self._is_cat_host is None
            and hasattr(self.backend, "DeviceGrower")
            and os.environ.get("SMXGB_NO_DEVICE_GROW") != "1"
            and os.environ.get("SMXGB_PIPELINE") != "v1"
            and p.grow_policy == "depthwise"
            and p.max_leaves == 0
            and 1 <= p.max_depth <= 10
            and p.colsample_bylevel >= 1.0
            and p.colsample_bynode >= 1.0
        )

    def _class_stream(self, slot):
        """One HIP stream per round-tree slot: a multiclass round's k small
        per-tree kernels (Covertype-shape trees underfill 256 CUs on their
        own) execute CONCURRENTLY across class streams instead of
        back-to-back on one stream."""
        streams = getattr(self, "_streams", None)
        if streams is None:
            streams = {}
            self._streams = streams
        # SMXGB_CLASS_STREAMS caps concurrent streams (slots share
        # round-robin); default one stream per slot
        cap = int(os.environ.get("SMXGB_CLASS_STREAMS", "0") or 0)
        key = slot % cap if cap > 0 else slot
        s = streams.get(key)
        if s is None:
            s = torch.cuda.Stream(device=self.device)
            streams[key] = s
        return s

    def grow_async(self, gh, slot=0):
        """Enqueue one independent tree of a round without waiting.

        Requires device_async_ok(). Each `slot` uses its own compact
        buffers, heap AND HIP stream, so several trees of one round
        (multiclass / bagging) run concurrently on the GPU.
        Returns an opaque handle for grow_finish().
        """
        p = self.p
        qm = self.qm
        n = qm.num_row
        self.grow_path = "device"
        # per-qm shared caches must exist on the DEFAULT stream before any
        # class stream reads them (class streams only order against the
        # default stream, not each other)
        if not getattr(qm, "_async_warm", False):
            if getattr(qm, "_arange_cache", None) is None or qm._arange_cache.numel() != n:
                qm._arange_cache = torch.arange(n, dtype=torch.int32, device=self.device)
            if not hasattr(qm, "_nbins_i32"):
                qm._nbins_i32 = qm.nbins.to(torch.int32).contiguous()
            qm._async_warm = True
        stream = self._class_stream(slot)
        stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(stream):
            rows, gh = self._sample_rows(gh)
            state = self.backend.make_tree_state(qm, gh, rows, slot=slot)
            state.margin_all_rows = self._gradient_sampled(None)
            self.state = state
            scale = self.backend.compute_scale(gh, comm=None)
            tree_mask = self._sample_features(p.colsample_bytree, None)
            dg = self._device_grower_for(slot)
            dg.state = state
            dg.traverse = self._traverse_ok(state)
            if tree_mask is not None:
                dg.mask = tree_mask.to(torch.uint8).contiguous()
            ev = dg.grow_enqueue(scale, (p.reg_lambda, p.reg_alpha, p.gamma, p.min_child_weight))
        return {"dg": dg, "ev": ev, "state": state, "cap": state.cap, "stream": stream,
                "rows": rows}

    def grow_finish(self, handle):
        """Wait for a grow_async tree and build its host Tree."""
        splits_np, counts_np, root_np = handle["dg"].grow_wait(handle["ev"])
        state = handle["state"]
        state._level0 = not bool(splits_np[0, 0] > 0)
        self.state = state  # so the caller's update_margins hits this slot
        self.tree_rows = handle["rows"]
        tree, leaf_jobs = self._build_tree_from_heap(
            splits_np, counts_np, root_np, handle["cap"]
        )
        self._bind_traverse(state, handle["dg"])
        tree.finalize()
        return tree, leaf_jobs

    def _build_tree_from_heap(self, splits_np, counts_np, root_np, cap):
        p = self.p
        qm = self.qm
        D = p.max_depth
        if not hasattr(qm, "_cuts_np"):
            qm._cuts_np = qm.cuts.cpu().numpy()
            qm._cut_ptr_np = qm.cut_ptr.cpu().numpy()

        tree = Tree()
        G, H = float(root_np[0]), float(root_np[1])
        root = tree.add_node(parent=-1, value=self._weight(G, H) * p.eta, sum_hess=H)
        leaf_jobs = []
        # heap index of each leaf_jobs entry. When margins are updated by
        # traversal the deepest level is not partitioned (nor, with the
        # filtered deepest histogram, the level above it): the counts of
        # levels D-2 and D-1 stay zero and the row ranges derived from them
        # below are placeholders nobody reads; the heap indices are what
        # that update uses.
        leaf_heap = []
        leaf_nodes = []  # tree node id of each leaf_jobs entry
        from collections import deque

        # this loop sits between one tree's readback and the next tree's
        # enqueue: unconstrained trees skip the bound bookkeeping
        monotone = self._monotone_host is not None
        unbounded = (-float("inf"), float("inf"))
        # BFS so node numbering matches the per-level path exactly; each
        # entry carries the node's monotone weight bounds
        stack = deque([(0, 0, root, 0, cap, G, H, unbounded)])
        while stack:
            d, i, nid, start, end, g, h, bounds = stack.popleft()
            hidx = (1 << d) - 1 + i
            gain = float(splits_np[hidx, 0]) if d < D else -1.0
            if d < D and gain > 0.0:
                feat = int(splits_np[hidx, 1])
                sbin = int(splits_np[hidx, 2])
                dl = bool(splits_np[hidx, 3] > 0.5)
                lg = float(splits_np[hidx, 4])
                lh = float(splits_np[hidx, 5])
                lc = int(counts_np[hidx, 0])
                threshold = float(qm._cuts_np[int(qm._cut_ptr_np[feat]) + sbin])
                if monotone:
                    wl, wr, lbounds, rbounds = self._child_weights(
                        feat, bounds[0], bounds[1], lg, lh, g - lg, h - lh
                    )
                else:
                    wl = self._weight(lg, lh)
                    wr = self._weight(g - lg, h - lh)
                    lbounds = rbounds = unbounded
                lid, rid = tree.apply_split(
                    nid, feat, threshold, sbin, dl, gain,
                    left_value=wl * p.eta,
                    right_value=wr * p.eta,
                    left_hess=lh,
                    right_hess=h - lh,
                )
                mid = start + lc
                stack.append((d + 1, 2 * i, lid, start, mid, lg, lh, lbounds))
                stack.append((d + 1, 2 * i + 1, rid, mid, end, g - lg, h - lh, rbounds))
            else:
                parity = 0 if d == 0 else d % 2
                leaf_jobs.append((parity, start, end, float(tree.value[nid])))
                leaf_heap.append(hidx)
                leaf_nodes.append(nid)
        self._leaf_heap = leaf_heap
        self.leaf_nodes = leaf_nodes
        # levels 0..D-1 that held a node: BFS pops the deepest node last
        self._live_levels = min(d + 1, D)
        return tree, leaf_jobs

    # -- depthwise ----------------------------------------------------------
    def _grow_depthwise(self, tree, gh, scale, root_node, tree_mask):
        p = self.p
        prev_hists = None  # previous level's fused hist tensor
        prev_row = {}      # nid -> row in prev_hists
        finished = []  # _Node leaves
        frontier = [root_node]
        n_leaves = 1
        depth = 0
        while frontier and (p.max_depth == 0 or depth < p.max_depth):
            if p.max_leaves and n_leaves >= p.max_leaves:
                break
            level_mask = self._sample_features(p.colsample_bylevel, tree_mask)

            # 1. histograms (smaller-by-global-hessian child built, sibling derived)
            build_nodes, derived = [], []
            for node in frontier:
                parent = int(tree.parent[node.nid])
                if parent < 0:
                    build_nodes.append(node)
                else:
                    sib_nid = (
                        int(tree.right[parent]) if int(tree.left[parent]) == node.nid else int(tree.left[parent])
                    )
                    sibling = next(m for m in frontier if m.nid == sib_nid)
                    if (node.h, node.nid) <= (sibling.h, sib_nid):
                        build_nodes.append(node)
                    else:
                        derived.append((node.nid, parent, sib_nid))

            # one fused level tensor: built rows copied in, derived rows =
            # prev-level parent minus sibling (single batched subtraction)
            frontier_row = {node.nid: i for i, node in enumerate(frontier)}
            slots = self.qm.total_slots
            hists = torch.empty((len(frontier), slots, 2), dtype=torch.float32, device=self.device)
            if build_nodes:
                acc = self.state.build_histograms(
                    [n.seg for n in build_nodes], build_nodes[0].parity, scale
                )
                self._allreduce(acc)
                built = self.backend.hist_to_float(acc, scale)
                build_rows = torch.tensor(
                    [frontier_row[n.nid] for n in build_nodes], dtype=torch.long, device=self.device
                )
                hists.index_copy_(0, build_rows, built)
            if derived:
                drows = torch.tensor([frontier_row[nid] for nid, _p, _s in derived],
                                     dtype=torch.long, device=self.device)
                prows = torch.tensor([prev_row[pnid] for _n, pnid, _s in derived],
                                     dtype=torch.long, device=self.device)
                srows = torch.tensor([frontier_row[snid] for _n, _p, snid in derived],
                                     dtype=torch.long, device=self.device)
                hists.index_copy_(
                    0, drows, prev_hists.index_select(0, prows) - hists.index_select(0, srows)
                )

            # 2. batched split search
            parent_sums = torch.tensor(
                [node.sum32 if node.sum32 is not None else (node.g, node.h) for node in frontier],
                dtype=torch.float32, device=self.device,
            )
            node_feature_mask = self._sample_features(p.colsample_bynode, level_mask)
            if any(node.allowed is not None for node in frontier):
                f = self.qm.num_col
                base = node_feature_mask if node_feature_mask is not None else torch.ones(
                    f, dtype=torch.bool, device=self.device
                )
                node_feature_mask = torch.stack([self._node_mask(base, node) for node in frontier])
            splits = self.backend.find_splits(
                hists,
                parent_sums,
                self.qm,
                reg_lambda=p.reg_lambda,
                reg_alpha=p.reg_alpha,
                gamma=p.gamma,
                min_child_weight=p.min_child_weight,
                feature_mask=node_feature_mask,
                monotone=self.monotone,
                **self._split_kwargs,
            )
            # 3. partition every positive-gain segment against the DEVICE
            # split tensor (no host round-trip before partitioning), then
            # read splits + counts back in a single queue drain
            parity = frontier[0].parity
            cat_kwargs = {"cat_bits": splits["cat_bits"]} if "cat_bits" in splits else {}
            counters = self.state.partition_level(
                [node.seg for node in frontier],
                list(range(len(frontier))),
                splits["packed"],
                parity,
                **cat_kwargs,
            )
            packed, cat_sets = self._read_splits(splits)  # the level's drain
            counts = counters[:, 0].cpu().tolist()
            gains = packed[:, 0]
            feats = packed[:, 1].astype(int)
            bins = packed[:, 2].astype(int)
            dls = packed[:, 3] > 0.5
            lgs = packed[:, 4]
            lhs = packed[:, 5]

            next_frontier = []
            for i, node in enumerate(frontier):
                if gains[i] <= 0.0 or (p.max_leaves and n_leaves >= p.max_leaves):
                    finished.append(node)
                    continue
                n_leaves += 1
                lid, rid, lstate, rstate = self._apply_split(
                    tree, node, int(feats[i]), int(bins[i]), bool(dls[i]),
                    float(gains[i]), float(lgs[i]), float(lhs[i]),
                    cat_bits=cat_sets[i] if cat_sets is not None else None,
                )
                mid = node.start + counts[i]
                mirror = node.sum32 is not None
                next_frontier.append(
                    _Node(lid, 1 - parity, node.start, mid, float(lgs[i]), float(lhs[i]),
                          depth + 1, lstate[0], lstate[1], lstate[2],
                          sum32=(lgs[i], lhs[i]) if mirror else None)
                )
                next_frontier.append(
                    _Node(
                        rid, 1 - parity, mid, node.end,
                        node.g - float(lgs[i]), node.h - float(lhs[i]), depth + 1,
                        rstate[0], rstate[1], rstate[2],
                        sum32=(node.sum32[0] - lgs[i], node.sum32[1] - lhs[i]) if mirror else None,
                    )
                )

            prev_hists = hists
            prev_row = frontier_row
            frontier = next_frontier
            depth += 1

        finished.extend(frontier)
        self.leaf_nodes = [n.nid for n in finished]
        return [(n.parity, n.start, n.end, float(tree.value[n.nid])) for n in finished]

    # -- lossguide ----------------------------------------------------------
    def _grow_lossguide(self, tree, gh, scale, root_node, tree_mask):
        p = self.p
        max_leaves = p.max_leaves if p.max_leaves else 2 ** max(p.max_depth, 1)
        node_hist = {}
        nodes = {root_node.nid: root_node}
        counter = 0
        heap = []

        def evaluate(node, sibling=None):
            nonlocal counter
            parent = int(tree.parent[node.nid])
            if node.nid not in node_hist:
                if parent >= 0 and sibling is not None and sibling.nid in node_hist:
                    self._build_level_hists(gh, scale, [], [(node.nid, parent, sibling.nid)], node_hist)
                else:
                    self._build_level_hists(gh, scale, [node], [], node_hist)
            mask = self._node_mask(self._sample_features(p.colsample_bynode, tree_mask), node)
            s = self.backend.find_splits(
                node_hist[node.nid].unsqueeze(0),
                torch.tensor([(node.g, node.h)], dtype=torch.float32, device=self.device),
                self.qm,
                reg_lambda=p.reg_lambda,
                reg_alpha=p.reg_alpha,
                gamma=p.gamma,
                min_child_weight=p.min_child_weight,
                feature_mask=mask,
                monotone=self.monotone,
                **self._split_kwargs,
            )
            packed_host, cat_host = self._read_splits(s)
            row = packed_host[0]
            gain = float(row[0])
            cat_dev = s.get("cat_bits")
            if gain > 0.0:
                heapq.heappush(
                    heap,
                    (
                        -gain,
                        counter,
                        node.nid,
                        {
                            "feature": int(row[1]),
                            "bin": int(row[2]),
                            "default_left": bool(row[3] > 0.5),
                            "left_g": float(row[4]),
                            "left_h": float(row[5]),
                            "gain": gain,
                            "packed_dev": s["packed"],
                            "cat_dev": cat_dev,
                            "cat_bits": cat_host[0] if cat_host is not None else None,
                        },
                    ),
                )
            counter += 1

        evaluate(root_node)
        n_leaves = 1
        split_ids = set()
        while heap and n_leaves < max_leaves:
            _neg, _c, nid, s = heapq.heappop(heap)
            node = nodes[nid]
            if p.max_depth and node.depth >= p.max_depth:
                continue
            cat_kwargs = {"cat_bits": s["cat_dev"]} if s["cat_dev"] is not None else {}
            counters = self.state.partition_level(
                [node.seg], [0], s["packed_dev"], node.parity, **cat_kwargs
            )
            counts = [int(counters[0, 0])]
            lid, rid, lstate, rstate = self._apply_split(
                tree, node, s["feature"], s["bin"], s["default_left"], s["gain"], s["left_g"], s["left_h"],
                cat_bits=s["cat_bits"],
            )
            mid = node.start + counts[0]
            lnode = _Node(lid, 1 - node.parity, node.start, mid, s["left_g"], s["left_h"],
                          node.depth + 1, lstate[0], lstate[1], lstate[2])
            rnode = _Node(
                rid, 1 - node.parity, mid, node.end, node.g - s["left_g"], node.h - s["left_h"],
                node.depth + 1, rstate[0], rstate[1], rstate[2]
            )
            nodes[lid] = lnode
            nodes[rid] = rnode
            split_ids.add(nid)
            del nodes[nid]
            n_leaves += 1
            # build smaller child first so the larger derives by subtraction
            first, second = (lnode, rnode) if lnode.h <= rnode.h else (rnode, lnode)
            evaluate(first, second)
            evaluate(second, first)
            node_hist.pop(nid, None)
        node_hist.clear()
        self.leaf_nodes = [n.nid for n in nodes.values()]
        return [(n.parity, n.start, n.end, float(tree.value[n.nid])) for n in nodes.values()]

    # -- shared ---------------------------------------------------------------
    @staticmethod
    def _read_splits(splits):
        """Host copies (packed [k, 6] float32, cat_bits [k, 8] int32 or None)
        of a find_splits result in ONE device readback: with categorical
        columns the two tensors travel as one [k, 14] int32 tensor (an
        integer copy keeps the float bit patterns)."""
        packed = splits["packed"]
        cat_bits = splits.get("cat_bits")
        if cat_bits is None:
            return packed.cpu().numpy(), None
        both = torch.cat(
            [packed.contiguous().view(torch.int32), cat_bits.to(torch.int32)], dim=1
        ).cpu().numpy()
        return np.ascontiguousarray(both[:, :6]).view(np.float32), both[:, 6:]

    def _child_weights(self, feature, lower, upper, left_g, left_h, right_g, right_h):
        """Child weights of a split under the parent's monotone weight
        bounds (lower, upper): a constrained feature pins the children to
        either side of the midpoint of their clamped weights. Returns
        (wl, wr, (l_lo, l_hi), (r_lo, r_hi))."""
        l_lo, l_hi = lower, upper
        r_lo, r_hi = lower, upper
        constraint = self._monotone_host[feature] if self._monotone_host is not None else 0
        wl = self._weight(left_g, left_h, lower, upper)
        wr = self._weight(right_g, right_h, lower, upper)
        if constraint != 0:
            mid = 0.5 * (wl + wr)
            if constraint > 0:
                l_hi = min(l_hi, mid)
                r_lo = max(r_lo, mid)
            else:
                l_lo = max(l_lo, mid)
                r_hi = min(r_hi, mid)
            wl = self._weight(left_g, left_h, l_lo, l_hi)
            wr = self._weight(right_g, right_h, r_lo, r_hi)
        return wl, wr, (l_lo, l_hi), (r_lo, r_hi)

    def _apply_split(self, tree, node, feature, bin_idx, default_left, gain, left_g, left_h,
                     cat_bits=None):
        """Apply one split: node values honor monotone bounds; returns
        (lid, rid, left_state, right_state) where each state is
        (lower, upper, allowed) for the child _Node. `cat_bits` is the
        split's category set, stored on the tree when `feature` is
        categorical."""
        p = self.p
        GR, HR = node.g - left_g, node.h - left_h
        if self._is_cat_host is not None and self._is_cat_host[feature]:
            cat_bits = np.asarray(cat_bits).astype(np.uint32)
            # the stored condition: the category of a one-hot split, else NaN
            threshold = float("nan")
            if self._nbins_host()[feature] < p.max_cat_to_onehot:
                threshold = float(cat_members(cat_bits)[0])
        else:
            cat_bits = None
            cut_base = int(self.qm.cut_ptr[feature])
            threshold = float(self.qm.cuts[cut_base + bin_idx])

        wl, wr, (l_lo, l_hi), (r_lo, r_hi) = self._child_weights(
            feature, node.lower, node.upper, left_g, left_h, GR, HR
        )

        child_allowed = self._interaction_allowed(node.allowed, feature)

        lid, rid = tree.apply_split(
            node.nid,
            feature,
            threshold,
            bin_idx,
            default_left,
            gain,
            left_value=wl * p.eta,
            right_value=wr * p.eta,
            left_hess=left_h,
            right_hess=HR,
            cat_bits=cat_bits,
        )
        return lid, rid, (l_lo, l_hi, child_allowed), (r_lo, r_hi, child_allowed)

    def _nbins_host(self):
        nb = getattr(self, "_nbins_list", None)
        if nb is None:
            nb = self._nbins_list = [int(v) for v in self.qm.nbins.tolist()]
        return nb
