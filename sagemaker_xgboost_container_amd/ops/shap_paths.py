"""Path tables for the path-form TreeSHAP kernels (host, plain numpy).

Every leaf becomes one path. Walking root -> leaf, all splits on the same
feature are merged into ONE element, so duplicate-feature handling is paid
once per model instead of once per row:

  feature        int32   split feature of the element
  lo, hi         f32     x follows the path iff lo <= x < hi, where lo is
                         the max threshold over right turns and hi the min
                         threshold over left turns on that feature
  flags          u8      FLAG_NAN: every split on the feature sends missing
                         values the way this path goes; FLAG_LO / FLAG_HI:
                         the path has a right / left turn on the feature
                         (kept explicit so +-inf inputs on a one-sided
                         element are classified like the traversal does)
  zero_fraction  f64     product of cover[child] / cover[parent] over the
                         merged splits (cover <= 0 -> 1, the host guard)

Paths are ordered by tree, so a tree range [t_begin, t_end) is the
contiguous path range tree_path_ptr[t_begin] : tree_path_ptr[t_end].
"""
import numpy as np

FLAG_NAN = 1
FLAG_LO = 2
FLAG_HI = 4


def make_shap_paths(trees, tree_info, weight_drop):
    """Build the path tables for `trees` (models.tree.Tree list).

    Returns a dict of numpy arrays:
      elem_feature/elem_lo/elem_hi/elem_flags/elem_zero_fraction  (E,)
      path_offset (P+1,) into the element arrays, path_value (P,) leaf value
      after the weight_drop scaling, path_tree (P,), path_cls (P,)
      tree_path_ptr (T+1,), tree_max_len (T,) longest path of the tree
      INCLUDING the dummy root element, tree_max_feature (T,) (-1: stump)
    """
    e_feat, e_lo, e_hi, e_flags, e_z = [], [], [], [], []
    p_off, p_val, p_tree, p_cls = [0], [], [], []
    tree_ptr = [0]
    tree_len = []
    tree_maxf = []
    for t, tree in enumerate(trees):
        tree.finalize()
        if getattr(tree, "has_categorical", False):
            # a path element is a threshold interval; a category set is not one
            raise NotImplementedError(
                "TreeSHAP path tables are not implemented for models with categorical splits"
            )
        left = tree.left
        right = tree.right
        feat = tree.feature
        thresh = tree.threshold
        defl = tree.default_left
        cover = np.asarray(tree.sum_hess, dtype=np.float32).astype(np.float64)
        scale = float(weight_drop[t]) if weight_drop else 1.0
        value = (tree.value * scale).astype(np.float32)
        cls = int(tree_info[t])
        max_len = 1
        max_f = -1
        # DFS; a path state is a list of merged elements in first-seen order:
        # [feature, lo, hi, flags, zero_fraction]
        stack = [(0, [])]
        while stack:
            nid, elems = stack.pop()
            l = int(left[nid])
            if l < 0:
                for el in elems:
                    e_feat.append(el[0])
                    e_lo.append(el[1])
                    e_hi.append(el[2])
                    e_flags.append(el[3])
                    e_z.append(el[4])
                p_off.append(len(e_feat))
                p_val.append(value[nid])
                p_tree.append(t)
                p_cls.append(cls)
                max_len = max(max_len, len(elems) + 1)
                continue
            r = int(right[nid])
            f = int(feat[nid])
            thr = np.float32(thresh[nid])
            dl = bool(defl[nid])
            c = cover[nid] if cover[nid] > 0 else 1.0
            max_f = max(max_f, f)
            # push right first so leaves come out in left-to-right order
            for child, is_left in ((r, False), (l, True)):
                zf = cover[child] / c
                nan_ok = dl == is_left
                new = [list(el) for el in elems]
                for el in new:
                    if el[0] == f:
                        break
                else:
                    el = [f, np.float32(-np.inf), np.float32(np.inf), FLAG_NAN, 1.0]
                    new.append(el)
                if is_left:
                    el[2] = min(el[2], thr)
                    el[3] |= FLAG_HI
                else:
                    el[1] = max(el[1], thr)
                    el[3] |= FLAG_LO
                if not nan_ok:
                    el[3] &= ~FLAG_NAN
                el[4] = el[4] * zf
                stack.append((child, new))
        tree_ptr.append(len(p_val))
        tree_len.append(max_len)
        tree_maxf.append(max_f)
    return {
        "elem_feature": np.asarray(e_feat, dtype=np.int32),
        "elem_lo": np.asarray(e_lo, dtype=np.float32),
        "elem_hi": np.asarray(e_hi, dtype=np.float32),
        "elem_flags": np.asarray(e_flags, dtype=np.uint8),
        "elem_zero_fraction": np.asarray(e_z, dtype=np.float64),
        "path_offset": np.asarray(p_off, dtype=np.int32),
        "path_value": np.asarray(p_val, dtype=np.float32),
        "path_tree": np.asarray(p_tree, dtype=np.int32),
        "path_cls": np.asarray(p_cls, dtype=np.int32),
        "tree_path_ptr": np.asarray(tree_ptr, dtype=np.int32),
        "tree_max_len": np.asarray(tree_len, dtype=np.int32),
        "tree_max_feature": np.asarray(tree_maxf, dtype=np.int32),
    }


def _range_elements(paths, f, t_begin, t_end):
    """Per path element of trees [t_begin, t_end): (first element id, tree
    index relative to t_begin, dense output column path_cls * (f + 1) +
    elem_feature), the last two as int64 arrays."""
    tree_ptr = paths["tree_path_ptr"]
    p0, p1 = int(tree_ptr[t_begin]), int(tree_ptr[t_end])
    off = paths["path_offset"]
    e0, e1 = int(off[p0]), int(off[p1])
    lens = np.diff(off[p0:p1 + 1]).astype(np.int64)
    tree = np.repeat(paths["path_tree"][p0:p1].astype(np.int64) - t_begin, lens)
    col = (
        np.repeat(paths["path_cls"][p0:p1].astype(np.int64), lens) * (f + 1)
        + paths["elem_feature"][e0:e1].astype(np.int64)
    )
    return e0, tree, col


def range_pairs(paths, f, t_begin, t_end):
    """Distinct (tree, column) pairs of trees [t_begin, t_end): two int64
    arrays (tree - t_begin, dense output column) sorted by tree, then
    column. There are at most as many as the range has split nodes."""
    _, tree, col = _range_elements(paths, f, t_begin, t_end)
    width = int(col.max()) + 1 if col.size else 1
    uniq = np.unique(tree * width + col)
    return uniq // width, uniq % width


def max_chunk_slots(pairs, trees_per_chunk):
    """max_c S_c of a uniform chunking, from range_pairs' output alone."""
    tree, col = pairs
    if tree.size == 0:
        return 0
    width = int(col.max()) + 1
    uniq = np.unique((tree // trees_per_chunk) * width + col)
    return int(np.bincount(uniq // width).max())


def make_shap_slots(paths, f, t_begin, t_end, trees_per_chunk):
    """Chunk-local phi slots of trees [t_begin, t_end) cut into chunks of
    `trees_per_chunk` trees (the last one may be short).

    Within a chunk every distinct (path_cls, elem_feature) pair gets one slot
    0 .. S_c-1, in ascending order of its dense output column
    cls * (f + 1) + feature. Returns a dict of numpy arrays and ints:
      elem_slot       int32, one per path element of the range (element ids
                      elem_base .. elem_base + len - 1): its chunk-local slot
      elem_base       first element id of the range
      chunk_slot_ptr  (C+1,) int32 offsets of the chunks' slots in the ragged
                      slot axis of length S = sum S_c
      slot_col        (S,) int64 dense output column of every ragged slot
      cols            (U,) int64 sorted distinct values of slot_col
      col_ptr         (U+1,) int32 and
      col_slots       (S,) int32: the ragged slots of cols[j], in ascending
                      chunk order, are col_slots[col_ptr[j]:col_ptr[j+1]]
      max_slots       max_c S_c (0 when no tree of the range splits)
      n_chunks, trees_per_chunk
    """
    if trees_per_chunk < 1:
        raise ValueError("trees_per_chunk must be at least 1")
    n_trees = len(paths["tree_path_ptr"]) - 1
    if not (0 <= t_begin <= t_end <= n_trees):
        raise ValueError(f"tree range [{t_begin}, {t_end}) out of bounds")
    T = t_end - t_begin
    C = (T + trees_per_chunk - 1) // trees_per_chunk
    e0, tree, col = _range_elements(paths, f, t_begin, t_end)
    chunk = tree // trees_per_chunk
    width = int(col.max()) + 1 if col.size else 1
    # ragged slot axis: distinct (chunk, column) pairs, chunk-major
    uniq, inverse = np.unique(chunk * width + col, return_inverse=True)
    slot_chunk = uniq // width
    slot_col = uniq % width
    S = int(uniq.shape[0])
    if S >= 2 ** 31:
        raise ValueError("slot axis does not fit int32 offsets")
    chunk_slot_ptr = np.zeros(C + 1, dtype=np.int64)
    np.cumsum(np.bincount(slot_chunk, minlength=C), out=chunk_slot_ptr[1:])
    elem_slot = inverse.reshape(-1).astype(np.int64) - chunk_slot_ptr[chunk]
    # per output column: its slots, ascending ragged index = ascending chunk
    col_slots = np.argsort(slot_col, kind="stable")
    cols, counts = np.unique(slot_col, return_counts=True)
    col_ptr = np.zeros(cols.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=col_ptr[1:])
    return {
        "elem_slot": elem_slot.astype(np.int32),
        "elem_base": e0,
        "chunk_slot_ptr": chunk_slot_ptr.astype(np.int32),
        "slot_col": slot_col.astype(np.int64),
        "cols": cols.astype(np.int64),
        "col_ptr": col_ptr.astype(np.int32),
        "col_slots": col_slots.astype(np.int32),
        "max_slots": int(np.diff(chunk_slot_ptr).max()) if C else 0,
        "n_chunks": C,
        "trees_per_chunk": int(trees_per_chunk),
    }


def range_limits(paths, t_begin, t_end):
    """(L, max_feature) of trees [t_begin, t_end): the longest path incl.
    the dummy root element, and the largest split feature (-1 if none)."""
    if t_end <= t_begin:
        return 1, -1
    return (
        int(paths["tree_max_len"][t_begin:t_end].max()),
        int(paths["tree_max_feature"][t_begin:t_end].max()),
    )
