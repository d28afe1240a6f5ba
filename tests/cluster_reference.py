"""The friends-of-friends cluster estimator of ``c21cm_bubble_clusters_grids`` (include/c21cm_grid.h; DESIGN section
4.11), restated in numpy: the spec the device code is held to, integer for integer.

``label_simple`` is the spec itself: a plain union-find over the adjacency exactly as the header writes it down, no
scipy.  ``label_fast`` gets the same answer from ``scipy.ndimage.label`` (open boundaries) plus a small union-find over
the pairs of cells that face each other across the periodic faces; the host tests hold the two to each other and to
known answers, and the GPU tests use the fast one on the larger boxes.
"""

import itertools

import numpy as np


def offsets_of(connectivity):
    """the offsets o in {-1, 0, 1}^3, o != 0, with at most ``connectivity`` non-zero components"""
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in o) <= connectivity]


def _periodic3(periodic):
    if np.ndim(periodic) == 0:
        return (bool(periodic),) * 3
    p = tuple(bool(x) for x in periodic)
    assert len(p) == 3
    return p


def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def _union(parent, a, b):
    a, b = _find(parent, a), _find(parent, b)
    if a != b:
        parent[max(a, b)] = min(a, b)


def _finish(labels_flat):
    """(labels, roots, sizes, stats) from the flat array of roots (-1 where not selected)"""
    sel = labels_flat >= 0
    roots, sizes = np.unique(labels_flat[sel], return_counts=True)
    roots, sizes = roots.astype(np.int64), sizes.astype(np.int64)
    if roots.size:
        k = int(np.argmax(sizes))  # the first maximum: ties take the smallest root
        stats = np.array([sel.sum(), roots.size, sizes[k], roots[k]], np.int64)
    else:
        stats = np.array([0, 0, 0, -1], np.int64)
    return labels_flat.astype(np.int32), roots, sizes, stats


def label_simple(mask, connectivity=1, periodic=True):
    """The spec.  ``mask``: bool (nx, ny, nz).  Returns ``(labels, roots, sizes, stats)``: int32 labels shaped as the
    mask (the smallest flat index of the cell's cluster, -1 where not selected), int64 roots ascending and their
    sizes, and stats = [n_selected, n_clusters, largest size, its root]."""
    mask = np.asarray(mask, bool)
    shape = mask.shape
    per = _periodic3(periodic)
    offs = offsets_of(connectivity)
    flat = mask.ravel()
    parent = list(range(flat.size))
    for p in np.flatnonzero(flat):
        idx = np.unravel_index(p, shape)
        for o in offs:
            q = []
            for a in range(3):
                v = int(idx[a]) + o[a]
                if per[a]:
                    v %= shape[a]
                elif v < 0 or v >= shape[a]:
                    q = None
                    break
                q.append(v)
            if q is None:
                continue
            j = (q[0] * shape[1] + q[1]) * shape[2] + q[2]
            if flat[j]:
                _union(parent, int(p), j)
    out = np.full(flat.size, -1, np.int64)
    for p in np.flatnonzero(flat):
        out[p] = _find(parent, int(p))
    labels, roots, sizes, stats = _finish(out)
    return labels.reshape(shape), roots, sizes, stats


def label_fast(mask, connectivity=1, periodic=True):
    """``label_simple`` by way of ``scipy.ndimage.label``: scipy's open-boundary partition, merged across the periodic
    faces (a face cell against the up to nine cells it touches on the opposite face, as the connectivity allows), and
    named by the smallest flat index of each cluster (``ndimage.minimum``)."""
    from scipy import ndimage

    mask = np.asarray(mask, bool)
    shape = mask.shape
    per = _periodic3(periodic)
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, connectivity))
    parent = np.arange(n + 1)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a in range(3):
        if not per[a]:
            continue
        last = np.take(lab, shape[a] - 1, axis=a)  # the face at n_a - 1, over the two other axes
        first = np.take(lab, 0, axis=a)
        others = [b for b in range(3) if b != a]
        for d0 in (-1, 0, 1):
            for d1 in (-1, 0, 1):
                if 1 + (d0 != 0) + (d1 != 0) > connectivity:
                    continue
                # the cell (n_a - 1, i, j) against (0, i + d0, j + d1), the shifts wrapping only on periodic axes
                f = first
                for k, d in ((0, d0), (1, d1)):
                    if d == 0:
                        continue
                    f = np.roll(f, -d, axis=k)
                    if not per[others[k]]:
                        edge = [slice(None), slice(None)]
                        edge[k] = slice(-1, None) if d > 0 else slice(0, 1)
                        f = f.copy()
                        f[tuple(edge)] = 0
                both = (last > 0) & (f > 0)
                pairs = np.unique(np.stack([last[both], f[both]], axis=1), axis=0)
                for x, y in pairs:
                    rx, ry = find(int(x)), find(int(y))
                    if rx != ry:
                        parent[max(rx, ry)] = min(rx, ry)
    comp = np.array([find(i) for i in range(n + 1)], np.int64)
    merged = comp[lab]
    out = np.full(mask.size, -1, np.int64)
    if n:
        index = np.unique(comp[1:])
        smallest = ndimage.minimum(np.arange(mask.size, dtype=np.int64).reshape(shape), merged, index)
        to_root = np.zeros(n + 1, np.int64)
        to_root[index] = np.asarray(smallest, np.int64)
        out = np.where(mask, to_root[merged], -1).ravel()
    labels, roots, sizes, stats = _finish(out)
    return labels.reshape(shape), roots, sizes, stats


def histograms(sizes, edges):
    """``(hist_n, hist_cells)``: the clusters with edges[i] <= size < edges[i + 1] and the sum of their cells"""
    edges = np.asarray(edges, np.int64)
    sizes = np.asarray(sizes, np.int64)
    n_bins = len(edges) - 1
    bins = np.digitize(sizes, edges) - 1
    ok = (bins >= 0) & (bins < n_bins)
    hist_n = np.bincount(bins[ok], minlength=n_bins).astype(np.int64)
    hist_cells = np.zeros(n_bins, np.int64)
    np.add.at(hist_cells, bins[ok], sizes[ok])
    return hist_n, hist_cells


def select_mask(field, threshold, select_below=True):
    v = np.asarray(field, np.float32).astype(np.float64)
    return v < threshold if select_below else v >= threshold
