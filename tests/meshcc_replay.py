"""The definition of nrf_mesh_components / nrf_filter_mesh in numpy -- TEST INFRASTRUCTURE ONLY -- written from the comment in
include/nerfhip.h, by a different algorithm from the library's: plain min-label propagation over the triangles to a fixed point (no
forest, no roots, no hooks), and a property checker of a labelling that shares no code with it.

tests/test_mesh_components_cpu.py holds host/meshcc_plan_check.cpp (csrc/nrf_meshcc_plan.h under the sanitizers) to this module, and
the GPU tests hold the kernels to it.  Everything is integers and copied float bits: every comparison is exact."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

KEEP_LARGEST = 1  # NRF_MESH_KEEP_LARGEST

Parts = namedtuple("Parts", "labels table sweeps")       # labels uint32 [nv]; table uint32 [nc][3] = (label, vertices, triangles)
Filtered = namedtuple("Filtered", "old_vertex old_triangle triangles kept_labels")  # old ids of the kept ones; remapped triangles


def _tri(triangles):
    return np.ascontiguousarray(triangles, np.int64).reshape(-1, 3)


def labels(n_vertices, triangles):
    """(label[v] = the smallest vertex id of v's component, sweeps): every sweep gives the three vertices of every triangle the
    smallest label among them, all triangles at once from the labels of the sweep before; the sweep that changes nothing ends it"""
    t = _tri(triangles)
    lab = np.arange(n_vertices, dtype=np.int64)
    sweeps = 0
    while True:
        sweeps += 1
        new = lab.copy()
        if len(t):
            low = lab[t].min(axis=1)
            np.minimum.at(new, t.reshape(-1), np.repeat(low, 3))
        if np.array_equal(new, lab):
            return lab.astype(np.uint32), sweeps
        lab = new


def parts(n_vertices, triangles):
    t = _tri(triangles)
    lab, sweeps = labels(n_vertices, t)
    uniq, n_v = np.unique(lab, return_counts=True)
    n_t = np.zeros(len(uniq), np.int64)
    if len(t):
        tl, tc = np.unique(lab[t[:, 0]], return_counts=True)
        n_t[np.searchsorted(uniq, tl)] = tc
    table = np.stack([uniq.astype(np.int64), n_v, n_t], axis=1).astype(np.uint32).reshape(-1, 3)
    return Parts(lab, table, sweeps)


def kept_labels(table, min_triangles, flags):
    """the labels of the components the keep rule keeps, ascending"""
    table = np.asarray(table, np.int64).reshape(-1, 3)
    keep = [int(row[0]) for row in table if int(row[2]) >= int(min_triangles)]
    if flags & KEEP_LARGEST and len(table):
        most = int(table[:, 2].max())
        largest = min(int(row[0]) for row in table if int(row[2]) == most)  # a tie goes to the smaller label
        keep = [lb for lb in keep if lb == largest]
    elif flags & KEEP_LARGEST:
        keep = []
    return keep


def filter_mesh(p, n_vertices, triangles, min_triangles=0, flags=0):
    t = _tri(triangles)
    keep = kept_labels(p.table, min_triangles, flags)
    lab = p.labels.astype(np.int64)
    kv = np.isin(lab, keep) if n_vertices else np.zeros(0, bool)
    kt = kv[t[:, 0]] if len(t) else np.zeros(0, bool)
    new_id = np.cumsum(kv) - kv  # the number of kept vertices with a smaller old id
    out = new_id[t[kt]].astype(np.uint32).reshape(-1, 3)
    return Filtered(np.nonzero(kv)[0].astype(np.uint32), np.nonzero(kt)[0].astype(np.uint32), out, keep)


# ---------------------------------------------------------------- property checker (nothing above is used below)
def check_parts(label, table, n_vertices, triangles):
    """what a labelling and its table have to be whatever made them.  (That two components are not one is what the three-labels
    rule cannot show: a labelling that is too fine passes it only if no triangle joins two of its classes, which is the rule.)"""
    label = np.asarray(label, np.int64).reshape(-1)
    table = np.asarray(table, np.int64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    assert len(label) == n_vertices
    v = np.arange(n_vertices)
    assert np.all(label <= v), "a label above its vertex"
    assert np.all(label[label] == label), "labels are not idempotent"
    if len(t):
        assert np.all(label[t[:, 0]] == label[t[:, 1]]) and np.all(label[t[:, 1]] == label[t[:, 2]]), "a triangle spans two labels"
    assert np.all(np.diff(table[:, 0]) > 0), "rows are not in ascending label"
    assert np.array_equal(table[:, 0], v[label == v]), "rows are not the roots"
    assert int(table[:, 1].sum()) == n_vertices and int(table[:, 2].sum()) == len(t), "counts do not sum to the mesh's"
    assert np.all(table[:, 1] >= 1)
