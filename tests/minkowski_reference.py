"""The spec of the Minkowski functionals (``c21cm_minkowski_grids``, include/c21cm_grid.h) in
numpy, one threshold at a time.

A box is the cubical complex of its cells: every cell is a closed cube with 6 faces, 12 edges and 8 vertices, shared
with its neighbours; the complex wraps on a periodic axis, and through an open face there is no cell.  An element is
in the set iff a selected cell contains it.  ``counts`` pads the open axes with one unselected layer on each side (so
that the elements on an open face are found from the layer beyond it), wraps with ``np.roll``, and ORs the mask over
the 1 / 2 / 4 / 8 cells that contain a cube / face / edge / vertex.  The device code finds all thresholds in one pass
from the levels of the cells; this file deliberately does not.
"""

import itertools

import numpy as np

KINDS = ("n3", "n2x", "n2y", "n2z", "n1x", "n1y", "n1z", "n0")


def periodic3(periodic):
    if np.ndim(periodic) == 0:
        return (bool(periodic),) * 3
    assert len(periodic) == 3
    return tuple(bool(p) for p in periodic)


def select_mask(field, threshold, below=True):
    v = np.asarray(field, np.float32).astype(np.float64)
    return v < threshold if below else v >= threshold


def _any_of(m, axes):
    """the OR of ``m`` over the cells at 0 and -1 along every axis of ``axes``"""
    out = np.zeros_like(m)
    for shift in itertools.product((0, 1), repeat=len(axes)):
        out |= np.roll(m, shift, axes) if axes else m
    return out


def counts(mask, periodic=True):
    """int64 (8,) = n3, n2x, n2y, n2z, n1x, n1y, n1z, n0 of the 3-D boolean ``mask``"""
    per = periodic3(periodic)
    m = np.asarray(mask, bool)
    assert m.ndim == 3
    m = np.pad(m, [(0, 0) if p else (1, 1) for p in per], constant_values=False)
    out = [m.sum()]
    out += [_any_of(m, (a,)).sum() for a in range(3)]  # the face perpendicular to a lies between two cells along a
    out += [_any_of(m, tuple(b for b in range(3) if b != a)).sum() for a in range(3)]  # the edge along a: 2 x 2 cells
    out.append(_any_of(m, (0, 1, 2)).sum())
    return np.array(out, np.int64)


def counts_of_field(field, thresholds, below=True, periodic=True):
    """int64 (T, 8): one mask per threshold"""
    return np.stack([counts(select_mask(field, t, below), periodic) for t in thresholds])


def levels(field, thresholds):
    """the number of thresholds <= v per cell"""
    return np.searchsorted(np.asarray(thresholds, np.float64), np.asarray(field, np.float32).astype(np.float64),
                           side="right")


def euler(c):
    c = np.asarray(c, np.int64)
    return c[..., 7] - c[..., 4:7].sum(-1) + c[..., 1:4].sum(-1) - c[..., 0]


def functionals(c, shape, lengths):
    """dict of chi, genus, v0..v3 (fp64) from counts (..., 8) of a box of ``shape`` cells and ``lengths``"""
    c = np.asarray(c, np.int64)
    n_cells = int(np.prod(shape, dtype=np.int64))
    cell = [float(l) / int(n) for l, n in zip(lengths, shape)]
    cell_volume = float(np.prod(cell))
    volume = n_cells * cell_volume
    area = [cell_volume / l for l in cell]
    n3, n2, n1 = c[..., 0], c[..., 1:4], c[..., 4:7]
    chi = euler(c)
    surface = sum(np.float64(area[a]) * (n2[..., a] - n3).astype(np.float64) for a in range(3))
    curvature = sum(np.float64(cell[a])
                    * (n1[..., a] - n2[..., (a + 1) % 3] - n2[..., (a + 2) % 3] + n3).astype(np.float64)
                    for a in range(3))
    return dict(chi=chi, genus=np.float64(1.0) - chi.astype(np.float64) / np.float64(2.0),
                v0=n3.astype(np.float64) / np.float64(n_cells),
                v1=np.float64(2.0) * surface / np.float64(9.0) / np.float64(volume),
                v2=np.float64(2.0) * curvature / np.float64(9.0) / np.float64(volume),
                v3=chi.astype(np.float64) / np.float64(volume))


def known_shapes():
    """(name, mask, periodic, counts or None, chi or None, n0 or None): sets whose answers are known by hand"""
    one = [1, 2, 2, 2, 4, 4, 4, 8]

    def box(shape, *cells):
        m = np.zeros(shape, bool)
        for c in cells:
            m[c] = True
        return m

    hollow = box((5, 5, 5))
    hollow[1:4, 1:4, 1:4] = True
    hollow[2, 2, 2] = False
    ring = box((5, 5, 3))
    ring[1:4, 1:4, 1] = True
    ring[2, 2, 1] = False
    full = np.ones((3, 4, 5), bool)
    corners = box((6, 6, 6), (0, 0, 0), (5, 5, 5))
    out = [("one cell, periodic", box((4, 5, 6), (1, 2, 3)), True, one, 1, 8),
           ("one cell, open", box((4, 5, 6), (1, 2, 3)), False, one, 1, 8),
           ("one cell in a corner, open", box((4, 5, 6), (0, 0, 5)), False, one, 1, 8),
           ("1x1x1 periodic", np.ones((1, 1, 1), bool), True, [1] * 8, 0, 1),
           ("1x1x1 open", np.ones((1, 1, 1), bool), False, one, 1, 8),
           ("one cell of 2x2x2 periodic", box((2, 2, 2), (1, 0, 1)), True, one, 1, 8),
           ("full periodic", full, True, None, 0, None),
           ("full open", full, False, None, 1, None),
           ("full open in z", full, (True, True, False), None, 0, None),
           ("hollow block", hollow, True, None, 2, None),
           ("hollow block, open", hollow, False, None, 2, None),
           ("ring", ring, True, None, 0, None),
           ("two cells at a corner", box((4, 4, 4), (1, 1, 1), (2, 2, 2)), True, None, 1, 15),
           ("far corners, periodic", corners, True, None, 1, 15),
           ("far corners, open", corners, False, None, 2, 16)]
    return out
