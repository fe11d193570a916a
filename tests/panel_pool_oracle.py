"""Float64 oracle, derived error bound and edge scenes for the two plan-driven poolings (csrc/bev_pool_mfma.hip,
csrc/bev_pool_panel.hip over bevpool.MfmaPoolPlan).  Plain numpy: nothing here needs a GPU.

The oracle.  ``oracle(depth, feat, rd, rf, rb, shape)`` pools point by point in float64: every product d_p f_p of two
float32 values is exact in float64 (48 significant bits), the sums carry ~1e-16 relative error, nothing beside the
2^-24 of the kernels under test.  It returns, per output element, ``want = sum d_p f_p``, ``mag = sum |d_p f_p|`` and,
per voxel, the point count ``n_v``.  Points whose ``rb`` lies outside [0, B Z Y X) are dropped, as the plan drops them.

The bound.  ``|got - want| <= gamma_k mag`` with gamma_k = k u / (1 - k u), u = 2^-24 (round to nearest, float32) and
k = n_v + P_t, where P_t = ceil(unique feature rows of the voxel's tile / 48) is the tile's panel count.  Derivation:
both kernels compute a voxel's channel as
    w_cell = d_1 + d_2 + ...                 (points of a cell in list order, float32 adds)
    acc    = fma(F[r], w_cell, acc)          (the voxel's cells in row order, panel after panel inside a unit)
    out    = slab_0 + slab_1 + ...           (the tile's units in slice order)
A term d_p f_p is therefore touched by
  * at most (points of its cell - 1) roundings in the cell weight (the product w F itself is exact inside the fma),
  * one rounding per fma from its own cell to the last cell of its voxel in the unit: at most the voxel's cell count,
    and a voxel of n_v points in cells of which this one holds m has at most n_v - m + 1 cells,
  * one rounding per later slab: at most (slices of the tile - 1), and a tile has at most P_t slices for any ``group``
    (a unit holds at least one panel).
That is never more than (m - 1) + (n_v - m + 1) + (P_t - 1) < n_v + P_t roundings, each a factor (1 + delta),
|delta| <= u, on a partial sum that contains the term; (1 + u)^k - 1 <= gamma_k (Higham, Accuracy and Stability of
Numerical Algorithms, lemma 3.1) gives the bound.  The zero entries of the dense W of the MFMA form add fma(0, F, acc) =
acc: no rounding.  No constant is measured from the kernels.  The float32 C oracle (a chain of n_v fmaf) obeys the same
bound with k = n_v.

The scenes.  Each is a function returning ``(rd, rf, rb)`` on the grid B=1, Z=2, Y=12, X=20 (2 x 3 tiles of 8 x 8 per
plane, ragged in both axes: tiles of 64, 64, 32, 32, 32 and 16 voxels), N_FEAT = 1000 feature rows, N_DEPTH = 4000 depth
entries.  The point list is permuted, then sorted stably by ``rb``; three points with ``rb`` = -1, n_vox and n_vox + 5
are appended.  Feature row 0 and depth entry 0 are referenced by nobody; rows / entries 1, 2, 3 only by the dropped
points.  ``make_inputs`` sets every row and entry that no KEPT point references to NaN: a kernel that reads one of them
into a sum shows it.  depth is in [0.25, 1) and |feat| in [0.5, 2): every point contributes at least 0.125 to every
channel of its voxel, a hundred times the largest bound (tests/test_panel_pool_oracle_host.py asserts it), so a dropped,
doubled or misrouted point cannot hide.
"""
import numpy as np

B, Z, Y, X = 1, 2, 12, 20
N_VOX = B * Z * Y * X
N_FEAT, N_DEPTH = 1000, 4000
KP = 48                      # rows per panel (ocrf_bev_pool_mfma_panel_rows)
TS, TV = 8, 64               # tile side, voxel slots per tile
TCX, TCY = (X + TS - 1) // TS, (Y + TS - 1) // TS
TPP = TCX * TCY              # tiles per plane
N_TILES = B * Z * TPP
U = 2.0 ** -24
MIN_TERM = 0.125             # smallest |d_p f_p| of make_inputs
CHANNELS = (64, 80, 96, 128)
SEEDS = (7, 8)               # make_inputs: inputs A and B of the GPU test
CELL_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25)
ROWS_PER_TILE = (1, 45, 47, 48, 49, 95, 96, 97, 0, 3, 50, 2)
UNIT_TILE_ROWS = {2: 384, 7: 385, 6: 768, 1: 769, 0: 816}       # tile -> unique rows
DENSE_TILES = {0: (8, 0), 1: (16, 0), 6: (8, 1), 7: (16, 1)}    # tile -> (rows shared by all 64 voxels, single-voxel rows)
_FIRST_ROW, _FIRST_DEPTH = 4, 4                                   # 0: nobody, 1..3: the dropped points


def grid_shape(c):
    return (B, Z, Y, X, c)


# ----------------------------------------------------------------------------------------------------------------
# oracle and bound
# ----------------------------------------------------------------------------------------------------------------
def kept_points(rd, rf, rb, n_vox=N_VOX):
    rd, rf, rb = (np.asarray(a).astype(np.int64) for a in (rd, rf, rb))
    keep = (rb >= 0) & (rb < n_vox)
    return rd[keep], rf[keep], rb[keep]


def oracle(depth, feat, rd, rf, rb, shape):
    """-> want (n_vox, C) float64, mag (n_vox, C) float64, n_v (n_vox,) int64: voxel rows, layout 2."""
    b, z, y, x, c = shape
    n_vox = b * z * y * x
    rd, rf, rb = kept_points(rd, rf, rb, n_vox)
    terms = depth[rd].astype(np.float64)[:, None] * feat[rf].astype(np.float64)
    want = np.zeros((n_vox, c), np.float64)
    mag = np.zeros((n_vox, c), np.float64)
    np.add.at(want, rb, terms)
    np.add.at(mag, rb, np.abs(terms))
    return want, mag, np.bincount(rb, minlength=n_vox)


def to_layout(rows, shape, layout):
    """Voxel rows (n_vox, C) -> layout 0 (B,C,Z,Y,X) / 1 (B,Z*C,Y,X) / 2 (n_vox, C)."""
    b, z, y, x, c = shape
    v = np.asarray(rows).reshape(b, z, y, x, c)
    if layout == 0:
        return np.ascontiguousarray(v.transpose(0, 4, 1, 2, 3))
    if layout == 1:
        return np.ascontiguousarray(v.transpose(0, 1, 4, 2, 3)).reshape(b, z * c, y, x)
    return np.ascontiguousarray(v).reshape(b * z * y * x, c)


def from_layout(flat, shape, layout):
    """A kernel's output in ``layout`` (any shape of B*C*Z*Y*X elements) -> voxel rows (n_vox, C)."""
    b, z, y, x, c = shape
    a = np.asarray(flat).reshape(-1)
    if layout == 0:
        a = a.reshape(b, c, z, y, x).transpose(0, 2, 3, 4, 1)
    elif layout == 1:
        a = a.reshape(b, z, c, y, x).transpose(0, 1, 3, 4, 2)
    return np.ascontiguousarray(a).reshape(b * z * y * x, c)


def tile_of(rb):
    """Voxel index -> (tile, voxel slot inside the tile)."""
    rb = np.asarray(rb).astype(np.int64)
    plane, inpl = rb // (Y * X), rb % (Y * X)
    y, x = inpl // X, inpl % X
    return plane * TPP + (y // TS) * TCX + x // TS, (y % TS) * TS + x % TS


def voxel_of(tile, v):
    """(tile, voxel slot) -> voxel index, -1 where the slot lies beyond the ragged grid."""
    tile, v = np.asarray(tile).astype(np.int64), np.asarray(v).astype(np.int64)
    plane, kt = tile // TPP, tile % TPP
    y, x = (kt // TCX) * TS + v // TS, (kt % TCX) * TS + v % TS
    return np.where((y < Y) & (x < X), plane * Y * X + y * X + x, -1)


def tile_slots(tile):
    """The voxel slots of ``tile`` that lie inside the grid."""
    v = np.arange(TV)
    return v[voxel_of(np.full(TV, tile), v) >= 0]


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def bound(mag, n_v, rf, rb):
    """gamma_(n_v + P_t) mag, element by element; 0 for a voxel without points."""
    s = structure(None, rf, rb)
    p_t = s['panels_per_tile'][tile_of(np.arange(N_VOX))[0]]
    return gamma(np.where(n_v > 0, n_v + p_t, 0))[:, None] * mag


# ----------------------------------------------------------------------------------------------------------------
# what a scene's rank vectors amount to, from numpy alone
# ----------------------------------------------------------------------------------------------------------------
def structure(rd, rf, rb):
    """Tiles, panels and cells of the kept points, as MfmaPoolPlan is documented to form them: a tile's unique feature
    rows ascending, KP per panel; a cell = the points of one (voxel, row)."""
    if rd is None:
        rd = np.zeros_like(np.asarray(rf))
    rd, rf, rb = kept_points(rd, rf, rb)
    tile, v = tile_of(rb)
    rows_per_tile = np.zeros(N_TILES, np.int64)
    slot = np.zeros(rf.size, np.int64)
    for t in range(N_TILES):
        m = tile == t
        u, inv = np.unique(rf[m], return_inverse=True)
        rows_per_tile[t] = u.size
        slot[m] = inv
    panels_per_tile = (rows_per_tile + KP - 1) // KP
    panel_off = np.cumsum(panels_per_tile) - panels_per_tile
    panel = panel_off[tile] + slot // KP
    n_panels = int(panels_per_tile.sum())
    cell_key = (panel * TV + v) * KP + slot % KP                     # voxel-major inside a panel, rows ascending
    cells, points_per_cell = np.unique(cell_key, return_counts=True)
    cell_panel, cell_pv = cells // (TV * KP), cells // KP
    cells_per_panel = np.bincount(cell_panel, minlength=n_panels)
    runs = np.bincount(cell_pv, minlength=n_panels * TV).reshape(n_panels, TV)     # cells of voxel slot v in panel p
    last_rows = np.where(rows_per_tile > 0, (rows_per_tile - 1) % KP + 1, 0)
    cell_tile = np.repeat(np.arange(N_TILES), panels_per_tile)[cell_panel]
    return dict(rows_per_tile=rows_per_tile, panels_per_tile=panels_per_tile, panel_off=panel_off, n_panels=n_panels,
                rows_in_last_panel=last_rows, points_per_cell=points_per_cell, cells_per_panel=cells_per_panel,
                longest_run=runs.max(1) if n_panels else np.zeros(0, np.int64), cell_panel=cell_panel,
                cell_voxel=voxel_of(cell_tile, cell_pv % TV))


def expected_units(s, group, unit_cost=None, max_unit_panels=8):
    """The unit cuts MfmaPoolPlan documents, tile by tile with a plain loop -> list per tile of (first panel, end panel).
    A unit holds consecutive panels of one tile, at most ``group``; with ``unit_cost`` a new unit also starts where
    floor(cost of the tile's panels before this one / unit_cost) changes, cost of a panel = 1 + its longest voxel run / 8.
    A tile without points is one unit without panels."""
    g = max(1, min(int(group), max_unit_panels))
    out = []
    for t in range(N_TILES):
        p0, n = int(s['panel_off'][t]), int(s['panels_per_tile'][t])
        if n == 0:
            out.append([(0, 0)])
            continue
        units, start, excl, in_bucket, bucket = [], p0, 0.0, 0, 0
        for p in range(p0, p0 + n):
            b = int(np.floor(excl / unit_cost)) if unit_cost is not None else 0
            if p > p0 and (b != bucket or in_bucket % g == 0):
                units.append((start, p))
                start = p
                if b != bucket:
                    in_bucket = 0
            bucket = b
            in_bucket += 1
            excl += 1.0 + float(s['longest_run'][p]) / 8.0
        units.append((start, p0 + n))
        out.append(units)
    return out


# ----------------------------------------------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------------------------------------------
class _Points:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rb, self.rf = [], []

    def add(self, tile, v, row, n=1):
        vox = int(voxel_of(tile, v))
        assert vox >= 0
        self.rb += [vox] * int(n)
        self.rf += [int(row)] * int(n)

    def rows(self, n):
        """n distinct feature rows, ascending, none of them 0..3 or the last (the `cells` scene's own)."""
        return np.sort(self.rng.choice(np.arange(_FIRST_ROW, N_FEAT - 1), int(n), replace=False))

    def finish(self):
        rng = self.rng
        rb, rf = np.array(self.rb, np.int64), np.array(self.rf, np.int64)
        rd = rng.integers(_FIRST_DEPTH, N_DEPTH, rb.size)
        perm = rng.permutation(rb.size)
        rb, rf, rd = rb[perm], rf[perm], rd[perm]
        order = np.argsort(rb, kind='stable')
        rb, rf, rd = rb[order], rf[order], rd[order]
        rb = np.concatenate((rb, [-1, N_VOX, N_VOX + 5]))
        rf = np.concatenate((rf, [1, 2, 3]))
        rd = np.concatenate((rd, [1, 2, 3]))
        return rd.astype(np.int32), rf.astype(np.int32), rb.astype(np.int32)


CELLS_ONE_VOXEL = (4, 9)           # (tile, voxel slot) of the voxel that owns 13 cells


def cells():
    """Points per cell at the forks of the cell sum: 3 | 4 (inline record | rd_sorted list), 8 | 9 and 16 | 17 (batches
    of kPB = 8), each as the only cell of a voxel and as one of 13 cells of a single voxel; the grid's last voxel; the
    last feature row."""
    p = _Points(101)
    slots = p.rng.choice(tile_slots(1), len(CELL_COUNTS), replace=False)
    for v, row, n in zip(slots, p.rows(len(CELL_COUNTS)), CELL_COUNTS):
        p.add(1, v, row, n)
    for row, n in zip(p.rows(len(CELL_COUNTS)), p.rng.permutation(CELL_COUNTS)):
        p.add(*CELLS_ONE_VOXEL, row, n)
    p.rb.append(N_VOX - 1)
    p.rf.append(N_FEAT - 1)
    return p.finish()


def rows():
    """Unique rows per tile around the panel size: 45 / 47 (zero-padded last k-step), 48 | 49 and 96 | 97 (a full last
    panel | one row into the next), an empty tile; every row in 1 to 3 voxels of 1 or 2 points."""
    p = _Points(102)
    for t, n in enumerate(ROWS_PER_TILE):
        slots = tile_slots(t)
        for row in p.rows(n):
            for v in p.rng.choice(slots, int(p.rng.integers(1, 4)), replace=False):
                p.add(t, v, row, p.rng.integers(1, 3))
    return p.finish()


def units():
    """Tiles of 8 | 9 and 16 | 17 panels (kMaxUnitPanels, the kSB = 8 slab batches at group = 1) and one of 816 rows;
    in each, one voxel owns all 48 rows of the first panel: that panel costs 7 of unit_cost = 8."""
    p = _Points(103)
    for t, n in UNIT_TILE_ROWS.items():
        slots = tile_slots(t)
        owner = slots[int(p.rng.integers(slots.size))]
        others = slots[slots != owner]
        for i, row in enumerate(p.rows(n)):
            if i < KP:
                p.add(t, owner, row)
            p.add(t, others[int(p.rng.integers(others.size))], row, p.rng.integers(1, 3))
    return p.finish()


def dense():
    """Panels of 512 | 513 cells (kCR * kBlock: the cells requested one panel ahead | one more from memory) and of
    1024 | 1025 (kCellCap: one LDS window | a second one)."""
    p = _Points(104)
    for t, (n, extra) in DENSE_TILES.items():
        rws = p.rows(n + extra)
        single = set(p.rng.choice(rws, extra, replace=False).tolist())
        for row in rws:
            if int(row) in single:
                p.add(t, int(p.rng.integers(TV)), row)
            else:
                for v in range(TV):
                    p.add(t, v, row)
    return p.finish()


SCENES = {'cells': cells, 'rows': rows, 'units': units, 'dense': dense}


def make_inputs(rd, rf, rb, c, seed):
    """depth (N_DEPTH,) in [0.25, 1), feat (N_FEAT, c) with |feat| in [0.5, 2) and random sign, float32; NaN in every
    entry / row that no kept point references."""
    rng = np.random.default_rng(seed)
    depth = np.minimum(rng.uniform(0.25, 1.0, N_DEPTH).astype(np.float32), np.float32(1.0 - 2.0 ** -24))
    feat = np.minimum(rng.uniform(0.5, 2.0, (N_FEAT, c)).astype(np.float32), np.float32(2.0 - 2.0 ** -23))
    feat *= rng.choice(np.array([-1.0, 1.0], np.float32), feat.shape)
    krd, krf, _ = kept_points(rd, rf, rb)
    dead_d, dead_f = np.ones(N_DEPTH, bool), np.ones(N_FEAT, bool)
    dead_d[krd] = False
    dead_f[krf] = False
    depth[dead_d] = np.nan
    feat[dead_f] = np.nan
    return depth, feat
