"""Float64 numpy oracle of the split search with categorical features, for
tests/test_categorical.py and tests/test_gpu_categorical.py. It is written
from the rule alone (numeric: cut after a bin; categorical: a set R of
categories that go right) and shares no code with the package."""
import numpy as np


def _score(g, h, lam, alpha):
    a = max(abs(g) - alpha, 0.0)
    return a * a / (h + lam)


def node_candidates(hist, parent, nbins, is_cat, has_missing, lam=1.0, alpha=0.0, gamma=0.0,
                    min_child_weight=1.0, max_cat_to_onehot=4, max_cat_threshold=64, mask=None):
    """Every valid candidate of one node, best first.

    hist: (f, stride, 2) float64; parent: (2,). Returns a list of
    (gain, feature, candidate, dir, R, left_g, left_h), R a frozenset for a
    categorical feature and None for a numeric one, sorted by descending
    gain, then ascending (feature, candidate, dir): the first entry is the
    split the search must return."""
    f, stride, _ = hist.shape
    hist = np.asarray(hist, dtype=np.float64)
    pg, ph = float(parent[0]), float(parent[1])
    pscore = _score(pg, ph, lam, alpha)
    out = []
    for j in range(f):
        if mask is not None and not mask[j]:
            continue
        nb = int(nbins[j])
        G = hist[j, :nb, 0]
        H = hist[j, :nb, 1]
        mg, mh = (hist[j, stride - 1, 0], hist[j, stride - 1, 1]) if has_missing else (0.0, 0.0)
        cands = []  # (candidate index, R, left_g, left_h) without missing
        if is_cat[j]:
            nonempty = [c for c in range(nb) if not (G[c] == 0 and H[c] == 0)]
            m = len(nonempty)
            if m < 2:
                continue
            tg, th = G.sum(), H.sum()
            if nb < max_cat_to_onehot:
                for c in nonempty:
                    cands.append((c, frozenset([c]), tg - G[c], th - H[c]))
            else:
                order = sorted(nonempty, key=lambda c: (G[c] / (H[c] + lam), c))
                sg = np.cumsum(G[order])
                sh = np.cumsum(H[order])
                for p in range(1, m):
                    if min(p, m - p) > max_cat_threshold:
                        continue
                    if p <= m - p:
                        cands.append((p - 1, frozenset(order[:p]), tg - sg[p - 1], th - sh[p - 1]))
                    else:
                        cands.append((p - 1, frozenset(order[p:]), sg[p - 1], sh[p - 1]))
        else:
            sg = np.cumsum(G)
            sh = np.cumsum(H)
            for b in range(nb - 1):
                cands.append((b, None, sg[b], sh[b]))
        for idx, R, lg, lh in cands:
            for d in (0, 1):
                gl = lg + (mg if d else 0.0)
                hl = lh + (mh if d else 0.0)
                gr, hr = pg - gl, ph - hl
                if hl < min_child_weight or hr < min_child_weight:
                    continue
                gain = 0.5 * (_score(gl, hl, lam, alpha) + _score(gr, hr, lam, alpha) - pscore) - gamma
                out.append((gain, j, idx, d, R, gl, hl))
    out.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
    return out


def gap(cands, has_missing=True):
    """Relative distance of the best gain to the second-best one. Without
    missing values the two directions of one cut are the same split with the
    same gain (the search returns dir 0): that twin is not a rival."""
    best = cands[0]
    for c in cands[1:]:
        if not has_missing and (c[1], c[2]) == (best[1], best[2]):
            continue
        return (best[0] - c[0]) / abs(best[0])
    return np.inf


def bits_of(R):
    """(8,) uint32 words of a category set."""
    bits = np.zeros(8, dtype=np.uint32)
    for c in R or ():
        bits[c >> 5] |= np.uint32(1 << (c & 31))
    return bits


def hist_from_rows(codes, g, h, nbins, stride, has_missing):
    """(f, stride, 2) float64 histogram of integer codes (n, f), -1 missing."""
    n, f = codes.shape
    hist = np.zeros((f, stride, 2), dtype=np.float64)
    for j in range(f):
        slot = np.where(codes[:, j] < 0, stride - 1, codes[:, j])
        assert has_missing or (codes[:, j] >= 0).all()
        assert (codes[:, j] < nbins[j]).all()
        hist[j, :, 0] = np.bincount(slot, weights=g, minlength=stride)
        hist[j, :, 1] = np.bincount(slot, weights=h, minlength=stride)
    return hist
