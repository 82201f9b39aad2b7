"""Seeded float32 clouds that reach the corners of the geometry searches (the cell grid of csrc/knn.hip shared by k-NN, ball
query and 3-NN; the Morton sort and box pruning of csrc/fps.hip) which the four clouds of test_gpu_ops.clouds -- all about
2 units wide and next to the origin -- never do.  A plain helper module: test_geometry_clouds_host.py asserts on the CPU what
test_gpu_geometry_edges.py relies on, and both take the k-NN cases from `knn_cases()` so that neither can drift.

kind        construction                                                      reaches
far         uniform [0,2)^3 + (1024, -2048, 512), rounded to fp32              stopping margin against the coordinate quantum
plane_z     uniform [0,2)^2, z = 0.75                                          nz = 1
plane_x     x = -0.5, uniform y, z                                             nx = 1: every x-run is one cell
line        uniform x in [0,2), y = 1, z = -3                                  ny = nz = 1
point       every row (0.3, -1.7, 5.0)                                         h = emax; every distance tied
clusters    half in a 0.01-box at the origin, half in one at (100,100,100)     cell-budget loop; empty cells
outlier     uniform [0,2)^3, last 5 rows = (50,50,50) + 0.01 u                 cell-budget loop; many shells for those rows
far_plane   plane_z + the offset of far                                        both
"""
import functools

import numpy as np

KINDS = ["far", "plane_z", "plane_x", "line", "point", "clusters", "outlier", "far_plane"]
UNTIED = ("far", "plane_z", "plane_x", "line", "far_plane")  # no query may tie there (asserted by the host test)
FAR_OFFSET = (1024.0, -2048.0, 512.0)
POINT = (0.3, -1.7, 5.0)
OUTLIER_ROWS = 5


def offset_of(kind):
    """what `far` and `far_plane` are shifted by, as float64 (zeros for the other kinds)"""
    return np.array(FAR_OFFSET if kind.startswith("far") else (0.0, 0.0, 0.0))


def cloud(kind, seed, n, outlier_rows=OUTLIER_ROWS):
    """(n, 3) float32; the uniform draws are float64, shifted in float64 and rounded to fp32 once"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 2.0, size=(n, 3))
    if kind == "far":
        p = u + offset_of(kind)
    elif kind in ("plane_z", "far_plane"):
        u[:, 2] = 0.75
        p = u + offset_of(kind)
    elif kind == "plane_x":
        u[:, 0] = -0.5
        p = u
    elif kind == "line":
        u[:, 1] = 1.0
        u[:, 2] = -3.0
        p = u
    elif kind == "point":
        p = np.tile(np.array(POINT), (n, 1))
    elif kind == "clusters":
        p = u * 0.005  # a 0.01-box
        p[n // 2:] += 100.0
    elif kind == "outlier":
        p = u
        r = min(outlier_rows, n)
        p[n - r:] = 50.0 + 0.01 * rng.uniform(0.0, 1.0, size=(r, 3))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p.astype(np.float32))


def outside_queries(seed, m, shift=None):
    """uniform in [-1,3)^3: about 7/8 of the rows fall outside a [0,2)^3 support box; `shift` (float64, added before the
    rounding to fp32) moves them along with a `far*` support"""
    q = np.random.default_rng(seed).uniform(-1.0, 3.0, size=(m, 3))
    if shift is not None:
        q = q + np.asarray(shift, dtype=np.float64)
    return np.ascontiguousarray(q.astype(np.float32))


def superset_queries(support, seed, m, shift=None):
    """the support rows first, then m - n rows of outside_queries: FeaturePropagation's unknown points"""
    n = support.shape[0]
    assert m >= n
    return np.ascontiguousarray(np.concatenate([support, outside_queries(seed, m - n, shift)], axis=0))


# ---------------------------------------------------------------------------------------------------------------------
# The k-NN cases of test_gpu_geometry_edges.py.  Seeds: a random fp32 cloud ties now and then (one query in 2048 of `far`
# at k = 32 with some seeds), and a tied query is handed to the heap replay, which would hide a wrong grid kernel; so the
# seeds below are, per kind, the first of 1, 2, 3, ... for which NO query of an untied case has two equal distances among its
# k+1 nearest at the largest k used (which covers the smaller ones); test_geometry_clouds_host.py asserts it.  `line` and
# `far_plane` tie most often (one coordinate decides, or a quantum of 1.2e-4 does) and need seeds 18 and 53.
# ---------------------------------------------------------------------------------------------------------------------
SELF_N = (2048, 2049)
SELF_K_GROUP = (4, 16, 32)  # kg_query_group_kernel
SELF_K_WAVE = 40            # kg_query_kernel
SELF_K_HEAP = 100           # knn_exact_kernel: amc3d_knnquery_uses_grid == 0
SELF_SEED = {"far": 1, "plane_z": 1, "plane_x": 1, "line": 18, "point": 1, "clusters": 1, "outlier": 1, "far_plane": 53}
APART_KINDS = ("far", "plane_z", "outlier")
APART_SEED = {"far": (1, 101), "plane_z": (1, 101), "outlier": (1, 101)}  # (support, queries)
RAGGED_SEED = 1
REUSE_KINDS = ("far", "outlier")
REUSE_SEED = {"far": 1, "outlier": 1}


class KnnCase:
    """one k-NN search: support `xyz` (n,3), queries `q` (None: the support itself), segment ends, k; `untied_rows` are the
    queries (a boolean mask over the m rows) that must not tie; `grid` is the route the case is about"""

    def __init__(self, name, k, xyz, q, off, qoff, untied_rows, grid):
        self.name, self.k, self.xyz, self.q, self.off, self.qoff = name, k, xyz, q, list(off), list(qoff)
        self.untied_rows, self.grid = untied_rows, grid

    @property
    def queries(self):
        return self.xyz if self.q is None else self.q


def _all(m, flag):
    return np.full(m, bool(flag))


@functools.lru_cache(maxsize=None)
def _cloud(kind, seed, n):
    return cloud(kind, seed, n)


def self_case(kind, n, k):
    xyz = _cloud(kind, SELF_SEED[kind], n)
    return KnnCase(f"self-{kind}-{n}-{k}", k, xyz, None, [n], [n], _all(n, kind in UNTIED), k <= 64)


def apart_case(kind):
    """6000 support points against 700 outside_queries (moved along with `far`), k = 16"""
    s, qs = APART_SEED[kind]
    xyz = _cloud(kind, s, 6000)
    q = outside_queries(qs, 700, offset_of(kind))
    return KnnCase(f"apart-{kind}", 16, xyz, q, [6000], [700], _all(700, kind in UNTIED), True)


def mixed_case(kind):
    """600 support rows and 100 outside_queries against the same 6000 points.  apart_case's cell size is calibrated on
    queries that are all far from the support, which leaves a handful of cells; here the sampled queries are mostly support
    rows, the cells are as small as in a self search, and the 100 outside rows start in a clamped cell and cross up to
    ~1.7 units of empty cells ring by ring"""
    s, qs = APART_SEED[kind]
    xyz = _cloud(kind, s, 6000)
    q = np.ascontiguousarray(np.concatenate([xyz[:600], outside_queries(qs, 100, offset_of(kind))]))
    return KnnCase(f"mixed-{kind}", 16, xyz, q, [6000], [700], _all(700, kind in UNTIED), True)


def ragged_case(first):
    """the first segment is `first` rows of `point`, the second 2049 rows of `far`: the grid's box spans both, so the point
    segment sits in one cell; with first = 10 < k placeholders (1e10, segment start) fill the tail of its rows"""
    xyz = np.ascontiguousarray(np.concatenate([_cloud("point", RAGGED_SEED, first), _cloud("far", RAGGED_SEED, 2049)]))
    n = first + 2049
    return KnnCase(f"ragged-{first}", 16, xyz, None, [first, n], [first, n], np.arange(n) >= first, True)


def reuse_cases(kind):
    """the loss's pattern on one 8192-point support: k = 25 self search, then k = 4 on every 4th point and k = 16 on every
    16th, all on the first search's grid"""
    n = 8192
    xyz = _cloud(kind, REUSE_SEED[kind], n)
    out = [KnnCase(f"reuse-{kind}-25", 25, xyz, None, [n], [n], _all(n, kind in UNTIED), True)]
    for k in (4, 16):
        q = np.ascontiguousarray(xyz[::k])
        out.append(KnnCase(f"reuse-{kind}-{k}", k, xyz, q, [n], [q.shape[0]], _all(q.shape[0], kind in UNTIED), True))
    return out


def knn_cases():
    """every k-NN case of the GPU file, by name"""
    cases = []
    for kind in KINDS:
        for n in SELF_N:
            for k in SELF_K_GROUP + (SELF_K_WAVE, SELF_K_HEAP):
                cases.append(self_case(kind, n, k))
    cases += [apart_case(kind) for kind in APART_KINDS] + [mixed_case(kind) for kind in APART_KINDS]
    cases += [ragged_case(300), ragged_case(10)]
    for kind in REUSE_KINDS:
        cases += reuse_cases(kind)
    return {c.name: c for c in cases}
