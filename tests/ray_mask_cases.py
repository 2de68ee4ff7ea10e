"""Integer rays for the ray mask of the probability-grid inserters (ForEachRayPixel in
csrc/ray_mask_2d.h, inlined by GridMissKernel and BatchMissKernel), and the way to hand them to the
shipped kernels exactly.  Shared by tests/test_ray_mask_cases.py (the list is what it claims to be;
the host restatement equals the reference on it) and tests/test_gpu_grid_exact.py (the device
against the host restatement).  No device code here.

A ray is (begin, end) in superscaled cells, 1000 to the pixel: sub-pixel i of pixel p is
1000 p + i, and the ray runs between the CENTRES of its two sub-pixels.  In doubled units a centre
is odd (2 i + 1) and a pixel border even (2000 c), so the ray through sub-pixel centres meets the
lattice corner (2000 c, 2000 r) only where y2_begin + (2000 c - x2_begin) dy / dx is a whole
multiple of 2000.  Two consequences the list is built around:
  - a slope dy / dx = p / q in lowest terms passes through corners only when p and q are both odd
    (odd + odd * p / q must be even).  The 2:1, 1:2, 3:2 and 2:3 rays from a pixel centre are in
    the list as rays that graze one row per column at a fixed offset, never through a corner;
    the `odd_slope` family (3:1, 1:3, 5:3, 3:5 from a sub-pixel next to a corner) is the one that
    passes through a corner every q columns;
  - the main diagonal passes through corners from sub-pixel (s, s), the anti-diagonal from
    (s, 999 - s).

Exact points.  FineIndex computes lround((max - double(p)) / (resolution / 1000) - 0.5).  With
resolution 1000 * 2**-13 and max_x = max_y = 128 the point max - (i + 0.5) * 2**-13 is exact in
float32 for every index i < 10**6 and comes back as exactly i (test_ray_mask_cases.py checks every
i), so a superscaled cell is a float32 point and any integer ray reaches the kernels through
`insert` and `insert_batch`.  Cell x comes from max_y - py and cell y from max_x - px.

Tiles.  Every ray has its own origin, so every ray is an insertion of its own: no returns, one
miss (the end), the origin at the begin.  Into unknown cells the non-zero cells are then the ray's
mask.  `pack` gives each ray a tile of one grid -- its pixels moved by a whole number of pixels,
one empty pixel around the neighbourhood -- so that thousands of rays share a grid and a download.
"""
import functools
import itertools
from dataclasses import dataclass

import numpy as np

SCALE = 1000
RESOLUTION = 1000 * 2.0 ** -13            # exact in float32 and float64
MAX_XY = 128.0
MAX_INDEX = 10 ** 6                       # superscaled indices below this are exact points
MAX_CELLS = MAX_INDEX // SCALE            # so a grid has at most this many cells a side

SWEEP_BEGIN_PIXEL = (4, 4)
SWEEP_BEGIN_SUBS = (0, 1, 499, 500, 999)
SWEEP_END_PIXELS = tuple(range(1, 8))
SWEEP_END_SUBS = (0, 1, 250, 499, 500, 750, 998, 999)
SWEEP_SAMPLE = 1500                       # of the rays that touch no corner
SWEEP_SEED = 20
SPANS = (1, 63, 64, 65, 127, 128, 129, 200)          # pixels between the two ends
LATTICE_COLUMNS = 130
LATTICE_SLOPES = ((2, 1), (1, 2), (3, 2), (2, 3))    # dy : dx
ODD_SLOPES = ((3, 1), (1, 3), (5, 3), (3, 5))        # dy : dx, both odd: through corners
STRUCTURED_FAMILIES = ("horizontal", "vertical", "diagonal", "anti_diagonal", "lattice_slope",
                       "odd_slope", "single_column", "one_subpixel_dx", "point", "pixel_edges")


def corner_crossings(begin, end, scale=SCALE):
    """The number of borders between two pixel columns at which the ray from the centre of
    sub-pixel `begin` to the centre of sub-pixel `end` passes exactly through a lattice corner.
    Exact integer arithmetic on the line itself; nothing of the mask algorithms."""
    (bx, by), (ex, ey) = (begin, end) if begin[0] <= end[0] else (end, begin)
    if bx == ex:
        return 0
    x2, y2 = 2 * bx + 1, 2 * by + 1                   # the begin's centre, in half sub-pixels
    dx, dy = ex - bx, ey - by
    count = 0
    for column in range(bx // scale + 1, ex // scale + 1):
        rise, rest = divmod((2 * scale * column - x2) * dy, dx)     # y at the border is y2 + rise
        if rest == 0 and (y2 + rise) % (2 * scale) == 0:
            count += 1
    return count


def corner_class(begin, end):
    """("given" or "reversed", "up" or "down"): whether the ray is listed with its ends in x order,
    and the sign of dy once they are.  None for dy == 0 and for rays inside one sub-pixel column."""
    order = "given" if begin[0] <= end[0] else "reversed"
    (bx, by), (ex, ey) = (begin, end) if begin[0] <= end[0] else (end, begin)
    if ey == by or ex == bx:
        return None
    return order, "up" if ey > by else "down"


@dataclass(frozen=True)
class Ray:
    name: str
    family: str
    begin: tuple                  # superscaled (x, y), pixels counted from 1 inside the tile
    end: tuple

    @property
    def tile(self):
        """(width, height) in pixels: the ends' pixels with one empty pixel all around."""
        return (max(self.begin[0], self.end[0]) // SCALE + 2,
                max(self.begin[1], self.end[1]) // SCALE + 2)


def _ray(name, family, begin, end):
    """The ray moved by whole pixels so that the lowest pixel of its ends is 1 in x and in y."""
    shift_x = SCALE * (1 - min(begin[0], end[0]) // SCALE)
    shift_y = SCALE * (1 - min(begin[1], end[1]) // SCALE)
    return Ray(name, family, (begin[0] + shift_x, begin[1] + shift_y),
               (end[0] + shift_x, end[1] + shift_y))


def _both_orders(name, family, begin, end):
    return [_ray(name, family, begin, end), _ray(name + "_reversed", family, end, begin)]


# ---- the sweep ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_all():
    """All 78 400 rays of the sweep as (begin, end, corner_crossings)."""
    out = []
    for bsx, bsy in itertools.product(SWEEP_BEGIN_SUBS, repeat=2):
        begin = (SWEEP_BEGIN_PIXEL[0] * SCALE + bsx, SWEEP_BEGIN_PIXEL[1] * SCALE + bsy)
        for px, py in itertools.product(SWEEP_END_PIXELS, repeat=2):
            for esx, esy in itertools.product(SWEEP_END_SUBS, repeat=2):
                end = (px * SCALE + esx, py * SCALE + esy)
                out.append((begin, end, corner_crossings(begin, end)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """Every exact-corner ray of the sweep, then a seeded sample of the others."""
    rays = sweep_all()
    corner = [k for k, r in enumerate(rays) if r[2] > 0]
    plain = [k for k, r in enumerate(rays) if r[2] == 0]
    rng = np.random.default_rng(SWEEP_SEED)
    sample = sorted(rng.choice(len(plain), SWEEP_SAMPLE, replace=False).tolist())
    out = [Ray("sweep_corner_%d" % k, "sweep_corner", rays[k][0], rays[k][1]) for k in corner]
    out += [Ray("sweep_%d" % plain[j], "sweep", rays[plain[j]][0], rays[plain[j]][1])
            for j in sample]
    return tuple(out)


# ---- the structured rays ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structured_cases():
    out = []
    mid = SCALE // 2
    for n in SPANS:
        far = n * SCALE
        out += _both_orders("horizontal_%d" % n, "horizontal", (mid, mid), (mid + far, mid))
        out += _both_orders("vertical_%d" % n, "vertical", (mid, mid), (mid, mid + far))
        # through a corner at every border: from sub-pixel (s, s), and (s, 999 - s)
        for s in (mid - 1, mid):
            out += _both_orders("diagonal_%d_from_%d" % (n, s), "diagonal", (s, s),
                                (s + far, s + far))
            out += _both_orders("anti_diagonal_%d_from_%d" % (n, s), "anti_diagonal",
                                (s, SCALE - 1 - s + far), (s + far, SCALE - 1 - s))
        # inside one pixel column, dx != 0
        for sign in (1, -1):
            out += _both_orders("single_column_%d_%s" % (n, "up" if sign > 0 else "down"),
                                "single_column", (100, mid), (900, mid + sign * far))
    across = (LATTICE_COLUMNS - 1) * SCALE
    for dy, dx in LATTICE_SLOPES:                    # from a pixel centre
        for sx, sy in itertools.product((1, -1), repeat=2):
            out += _both_orders("lattice_slope_%d_%d_%s%s" % (dy, dx, "+-"[sx < 0], "+-"[sy < 0]),
                                "lattice_slope", (mid, mid),
                                (mid + sx * across, mid + sy * (across * dy // dx)))
    for dy, dx in ODD_SLOPES:
        # One step (dx, dy) in half sub-pixels short of the corner (0, 0) -- both odd, so a
        # sub-pixel centre -- the ray passes through a corner every dx columns.
        steps = across // dx
        for sign in (1, -1):
            begin = ((-dx - 1) // 2, (-sign * dy - 1) // 2)
            out += _both_orders("odd_slope_%d_%d_%s" % (dy, dx, "up" if sign > 0 else "down"),
                                "odd_slope", begin,
                                (begin[0] + dx * steps, begin[1] + sign * dy * steps))
    # dx of one sub-pixel across a column border, |dy| of 200 pixels; and the same ending in the
    # next pixel at the sub-pixel that makes the crossing of the border a corner (the border is
    # half way: 2 mid + 1 + dy must be a multiple of 2000)
    for sign in (1, -1):
        tag = "up" if sign > 0 else "down"
        out += _both_orders("one_subpixel_dx_%s" % tag, "one_subpixel_dx", (SCALE - 1, mid),
                            (SCALE, mid + sign * 200 * SCALE))
        dy = sign * 202 * SCALE - (2 * mid + 1)
        out += _both_orders("one_subpixel_dx_%s_corner" % tag, "one_subpixel_dx",
                            (SCALE - 1, mid), (SCALE, mid + dy))
    for s in (0, mid, SCALE - 1):
        out.append(_ray("point_%d" % s, "point", (s, s), (s, s)))
    edges = (0, SCALE - 1)
    for bsx, bsy, esx, esy in itertools.product(edges, repeat=4):
        for rise in (3, -3):
            out += _both_orders("pixel_edges_%d_%d_%d_%d_%s" % (bsx, bsy, esx, esy,
                                                                "up" if rise > 0 else "down"),
                                "pixel_edges", (bsx, bsy), (5 * SCALE + esx, rise * SCALE + esy))
    assert len({r.name for r in out}) == len(out)
    return tuple(out)


# ---- exact points and tiles ---------------------------------------------------------------------
def points_of(fine_xy):
    """float32 xyz map points whose FineIndex is exactly the superscaled cells `fine_xy` [n, 2]
    on a grid of RESOLUTION with max_x = max_y = MAX_XY (cell x from y, cell y from x)."""
    fine = np.asarray(fine_xy, np.int64).reshape(-1, 2)
    assert fine.min(initial=0) >= 0 and fine.max(initial=0) < MAX_INDEX
    out = np.zeros((fine.shape[0], 3), np.float64)
    out[:, 0] = MAX_XY - (fine[:, 1] + 0.5) * 2.0 ** -13
    out[:, 1] = MAX_XY - (fine[:, 0] + 0.5) * 2.0 ** -13
    as_f32 = out.astype(np.float32)
    assert (as_f32.astype(np.float64) == out).all()
    return as_f32


@dataclass(frozen=True)
class Placed:
    ray: Ray
    grid: int                     # which grid of the layout
    x: int                        # the tile's corner, in pixels of that grid
    y: int

    @property
    def begin(self):
        return (self.ray.begin[0] + SCALE * self.x, self.ray.begin[1] + SCALE * self.y)

    @property
    def end(self):
        return (self.ray.end[0] + SCALE * self.x, self.ray.end[1] + SCALE * self.y)


@dataclass(frozen=True)
class Layout:
    sizes: tuple                  # (num_x_cells, num_y_cells) of every grid
    placed: tuple                 # Placed, in the order of the rays given


def pack(rays, grids=1):
    """Ray k goes to grid k % grids; inside a grid the tiles stand in rows, the tall ones first
    (a long ray ends up in a row of its like).  Every grid fits MAX_CELLS a side."""
    placed = [None] * len(rays)
    sizes = []
    for g in range(grids):
        mine = sorted(range(g, len(rays), grids), key=lambda k: (-rays[k].tile[1], k))
        x = y = row_height = width = 0
        for k in mine:
            w, h = rays[k].tile
            if x + w > MAX_CELLS:
                x, y, row_height = 0, y + row_height, 0
            placed[k] = Placed(rays[k], g, x, y)
            x, row_height, width = x + w, max(row_height, h), max(width, x + w)
        sizes.append((max(width, 1), max(y + row_height, 1)))
        assert sizes[-1][0] <= MAX_CELLS and sizes[-1][1] <= MAX_CELLS, (g, sizes[-1])
    return Layout(tuple(sizes), tuple(placed))
