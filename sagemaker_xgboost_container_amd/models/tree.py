"""Regression-tree structure (xgboost-layout-compatible).

Node arrays use xgboost conventions so serialization maps 1:1 onto the
Booster JSON schema ("left_children"/"right_children"/"split_indices"/
"split_conditions"/"default_left"/"base_weights"/"loss_changes"/
"sum_hessian"): leaf iff left < 0; test `fvalue < threshold` goes left.

A categorical node (split_type 1) holds a set R of categories that go
RIGHT as 256 bits in 8 uint32 words (`cat_bits`; bit c & 31 of word c >> 5);
the words of a numeric node are zero. `cat_goes_left` is the decision rule.

Construction uses Python lists (O(1) append — the grower adds two nodes per
split in the hot loop); `finalize()` converts to numpy arrays once when the
tree is done.
"""
import numpy as np

CAT_WORDS = 8                  # uint32 words of a node's category set
MAX_CAT = 32 * CAT_WORDS       # categories are the integers [0, MAX_CAT)


def cat_goes_left(fv, bits):
    """Decision at a categorical node for a non-missing value `fv` (the
    caller sends NaN the default way): a value outside [0, 256) goes left;
    otherwise the category is fv truncated, and members of the set go right."""
    if not (fv >= 0.0) or fv >= MAX_CAT:
        return True
    c = int(fv)
    return not ((int(bits[c >> 5]) >> (c & 31)) & 1)


def cat_bits_from_members(members):
    """(8,) uint32 bitset of an iterable of categories in [0, 256)."""
    bits = np.zeros(CAT_WORDS, dtype=np.uint32)
    for c in members:
        c = int(c)
        if not 0 <= c < MAX_CAT:
            raise ValueError(f"category {c} outside [0, {MAX_CAT})")
        bits[c >> 5] |= np.uint32(1 << (c & 31))
    return bits


def cat_members(bits):
    """Ascending list of the categories set in an (8,) uint32 bitset."""
    return [c for c in range(MAX_CAT) if (int(bits[c >> 5]) >> (c & 31)) & 1]


class Tree:
    def __init__(self):
        self.left = []
        self.right = []
        self.parent = []
        self.feature = []
        self.threshold = []      # split condition (fvalue < t -> left)
        self.split_bin = []      # training-time bin index of the split
        self.default_left = []
        self.value = []          # leaf value / base weight
        self.gain = []
        self.sum_hess = []
        self.split_type = []     # 0 numeric, 1 categorical
        self.cat_bits = []       # per node: None (numeric) or (8,) uint32 set
        self._finalized = False

    _FIELDS = (
        ("left", np.int32),
        ("right", np.int32),
        ("parent", np.int32),
        ("feature", np.int32),
        ("threshold", np.float32),
        ("split_bin", np.int32),
        ("default_left", bool),
        ("value", np.float32),
        ("gain", np.float32),
        ("sum_hess", np.float32),
        ("split_type", np.uint8),
    )

    def finalize(self):
        """Convert construction lists to numpy arrays (idempotent)."""
        if not self._finalized:
            for name, dtype in self._FIELDS:
                setattr(self, name, np.asarray(getattr(self, name), dtype=dtype))
            bits = np.zeros((len(self.left), CAT_WORDS), dtype=np.uint32)
            for nid in np.flatnonzero(self.split_type):
                bits[nid] = self.cat_bits[nid]
            self.cat_bits = bits
            self._finalized = True
        return self

    def _editable(self):
        if self._finalized:
            for name, _dtype in self._FIELDS:
                setattr(self, name, list(getattr(self, name)))
            self.cat_bits = [
                row.copy() if t else None for t, row in zip(self.split_type, self.cat_bits)
            ]
            self._finalized = False

    def __setstate__(self, state):
        # pickles from before categorical splits carry neither field
        self.__dict__.update(state)
        if "split_type" not in state:
            n = len(self.left)
            if self._finalized:
                self.split_type = np.zeros(n, dtype=np.uint8)
                self.cat_bits = np.zeros((n, CAT_WORDS), dtype=np.uint32)
            else:
                self.split_type = [0] * n
                self.cat_bits = [None] * n

    @property
    def has_categorical(self):
        return bool(np.any(np.asarray(self.split_type)))

    @property
    def num_nodes(self):
        return len(self.left)

    def is_leaf(self, nid):
        return self.left[nid] < 0

    @property
    def num_leaves(self):
        if self._finalized:
            return int((self.left < 0).sum())
        return sum(1 for v in self.left if v < 0)

    def add_node(self, parent=-1, value=0.0, sum_hess=0.0):
        """Append a leaf node; returns its id."""
        self._editable()
        nid = len(self.left)
        self.left.append(-1)
        self.right.append(-1)
        self.parent.append(parent)
        self.feature.append(0)
        self.threshold.append(0.0)
        self.split_bin.append(-1)
        self.default_left.append(False)
        self.value.append(float(value))
        self.gain.append(0.0)
        self.sum_hess.append(float(sum_hess))
        self.split_type.append(0)
        self.cat_bits.append(None)
        return nid

    def apply_split(self, nid, feature, threshold, split_bin, default_left, gain,
                    left_value, right_value, left_hess, right_hess, cat_bits=None):
        """Turn leaf `nid` into an internal node; returns (left_id, right_id).
        `cat_bits` ((8,) uint32: the categories that go right) makes it a
        categorical node."""
        lid = self.add_node(parent=nid, value=left_value, sum_hess=left_hess)
        rid = self.add_node(parent=nid, value=right_value, sum_hess=right_hess)
        self.left[nid] = lid
        self.right[nid] = rid
        self.feature[nid] = int(feature)
        self.threshold[nid] = float(threshold)
        self.split_bin[nid] = int(split_bin)
        self.default_left[nid] = bool(default_left)
        self.gain[nid] = float(gain)
        if cat_bits is not None:
            self.split_type[nid] = 1
            self.cat_bits[nid] = np.asarray(cat_bits).astype(np.uint32).reshape(CAT_WORDS).copy()
        return lid, rid

    def depth(self, nid):
        d = 0
        while self.parent[nid] >= 0:
            nid = self.parent[nid]
            d += 1
        return d

    def max_depth(self):
        return max((self.depth(n) for n in range(self.num_nodes) if self.is_leaf(n)), default=0)

    def predict_row(self, x, missing_is_nan=True):
        """Scalar traversal (host; for tests/debug)."""
        nid = 0
        while self.left[nid] >= 0:
            fv = x[self.feature[nid]]
            if np.isnan(fv):
                nid = self.left[nid] if self.default_left[nid] else self.right[nid]
            elif self.split_type[nid]:
                go_left = cat_goes_left(fv, self.cat_bits[nid])
                nid = self.left[nid] if go_left else self.right[nid]
            else:
                nid = self.left[nid] if fv < self.threshold[nid] else self.right[nid]
        return float(self.value[nid])

    def to_arrays(self):
        """Flat dict of node arrays (device-upload / serialization form)."""
        self.finalize()
        return {
            "left": self.left,
            "right": self.right,
            "parent": self.parent,
            "feature": self.feature,
            "threshold": self.threshold,
            "default_left": self.default_left,
            "value": self.value,
            "gain": self.gain,
            "sum_hess": self.sum_hess,
            "split_type": self.split_type,
            "cat_bits": self.cat_bits,
        }

    @classmethod
    def from_arrays(cls, arrays):
        t = cls()
        n = len(arrays["left"])
        t.left = np.asarray(arrays["left"], dtype=np.int32)
        t.right = np.asarray(arrays["right"], dtype=np.int32)
        t.parent = np.asarray(arrays.get("parent", np.full(n, -1)), dtype=np.int32)
        t.feature = np.asarray(arrays["feature"], dtype=np.int32)
        t.threshold = np.asarray(arrays["threshold"], dtype=np.float32)
        t.split_bin = np.asarray(arrays.get("split_bin", np.full(n, -1)), dtype=np.int32)
        t.default_left = np.asarray(arrays["default_left"], dtype=bool)
        t.value = np.asarray(arrays["value"], dtype=np.float32)
        t.gain = np.asarray(arrays.get("gain", np.zeros(n)), dtype=np.float32)
        t.sum_hess = np.asarray(arrays.get("sum_hess", np.zeros(n)), dtype=np.float32)
        t.split_type = np.asarray(arrays.get("split_type", np.zeros(n)), dtype=np.uint8)
        t.cat_bits = np.asarray(
            arrays.get("cat_bits", np.zeros((n, CAT_WORDS))), dtype=np.uint32
        ).reshape(n, CAT_WORDS)
        t._finalized = True
        return t
