"""Reference for cmpc_mask_components (include/cmpc.h) in plain NumPy, and the masks its tests use.

labels(mask, c): a stack flood fill in raster order.  The fill that starts at the first pixel of a component in raster order labels the
whole component 1 + that pixel's raster index: background 0, foreground 1 + min{y * w + x} over the component -- the canonical form.
clean(mask, keep, min_area, c): components ranked by area descending, ties to the smaller first-pixel index; one is kept iff
(keep == 0 or rank < keep) and area >= min_area; kept pixels keep their byte, other foreground pixels become 0;
stats = (n_components, area, area_largest, area_kept).  Shares no helper with hostutil.clean_mask."""
import numpy as np

DENSITIES = (0.3, 0.41, 0.5, 0.59, 0.7)
NOISE_SHAPE = (97, 131)
PATTERNS = ("empty", "full", "checkerboard", "diagonal", "antidiagonal", "serpentine", "comb", "comb_tm", "two_rectangles", "corner_touch")
KEEPS, MIN_AREAS = (0, 1, 2, 8), (0, 2, 50)


def labels(mask, connectivity: int) -> np.ndarray:
    m = np.asarray(mask) != 0
    h, w = m.shape
    if connectivity == 4:
        nbrs = ((-1, 0), (0, -1), (0, 1), (1, 0))
    elif connectivity == 8:
        nbrs = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
    else:
        raise ValueError(connectivity)
    out = np.zeros((h, w), np.int32)
    fg = m.tolist()
    seen = [[False] * w for _ in range(h)]
    for y0 in range(h):
        for x0 in range(w):
            if not fg[y0][x0] or seen[y0][x0]:
                continue
            lab, stack = 1 + y0 * w + x0, [(y0, x0)]
            seen[y0][x0] = True
            while stack:
                y, x = stack.pop()
                out[y, x] = lab
                for dy, dx in nbrs:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and fg[yy][xx] and not seen[yy][xx]:
                        seen[yy][xx] = True
                        stack.append((yy, xx))
    return out


def clean(mask, keep: int, min_area: int, connectivity: int, lab=None):
    """(cleaned mask, int64 stats [4], labels).  lab: labels(mask, connectivity) when the caller has them already."""
    a = np.asarray(mask)
    lab = labels(a, connectivity) if lab is None else lab
    ids, areas = np.unique(lab[lab > 0], return_counts=True)
    comps = sorted(zip(ids.tolist(), areas.tolist()), key=lambda c: (-c[1], c[0]))
    kept = [i for rank, (i, ar) in enumerate(comps) if (keep == 0 or rank < keep) and ar >= min_area]
    keep_px = np.isin(lab, kept)
    out = np.where(keep_px, a, 0).astype(a.dtype)
    stats = np.array([len(comps), int(areas.sum()), comps[0][1] if comps else 0, int(keep_px.sum())], np.int64)
    return out, stats, lab


def shapes(TH: int, TW: int):
    return [(1, 1), (1, 70), (70, 1), (2, 2), (7, 65), (TH, TW), (TH - 1, 2 * TW - 1), (TH + 1, 2 * TW + 1), (3 * TH + 5, 3 * TW + 7)]


def serpentine(h: int, w: int) -> np.ndarray:
    """One pixel wide: every even row, joined to the next by one pixel at alternating ends."""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for y in range(1, h, 2):
        m[y, w - 1 if (y // 2) % 2 == 0 else 0] = True
    return m


def comb(h: int, w: int) -> np.ndarray:
    """Teeth in every second column from the first row down, joined only along the last row."""
    m = np.zeros((h, w), bool)
    m[:, 0::2] = True
    m[h - 1] = True
    return m


def pattern(kind: str, h: int, w: int, TH: int, TW: int) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "empty":
        return np.zeros((h, w), bool)
    if kind == "full":
        return np.ones((h, w), bool)
    if kind == "checkerboard":
        return (yy + xx) % 2 == 0
    if kind == "diagonal":
        return yy == xx
    if kind == "antidiagonal":
        return yy == (w - 1 - xx)
    if kind == "serpentine":
        return serpentine(h, w)
    if kind == "comb":
        return comb(h, w)
    if kind == "comb_tm":                          # transposed and mirrored: teeth along the rows, joined along the first column
        return np.ascontiguousarray(comb(w, h).T[::-1, ::-1])
    if kind == "two_rectangles":                   # equal areas: the tie goes to the first in raster order
        rh, rw = max(h // 3, 1), max(w // 3, 1)
        m = np.zeros((h, w), bool)
        m[h - rh:, :rw] = True                     # the lower-left one comes second in raster order
        m[:rh, w - rw:] = True
        return m
    if kind == "corner_touch":                     # two rectangles that meet only at a tile corner
        m = np.zeros((h, w), bool)
        m[max(TH - 4, 0): TH, max(TW - 5, 0): TW] = True
        m[TH: TH + 3, TW: TW + 6] = True
        return m
    raise ValueError(kind)


def noise(density: float, shape=NOISE_SHAPE, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).random(shape) < density


def all_inputs(TH: int, TW: int):
    """[(name, bool mask)]: every pattern at every shape, and noise at the five densities."""
    out = [("%s %dx%d" % (k, h, w), pattern(k, h, w, TH, TW)) for k in PATTERNS for h, w in shapes(TH, TW)]
    return out + [("noise %.2f" % p, noise(p)) for p in DENSITIES]


def closed_form_frame(h: int, w: int):
    """A frame whose answer follows from its construction (h % 4 == 0, w % 8 == 0, w >= 32, h >= 12).  Left half: a serpentine over
    columns 0 .. w/2 - 2.  Right half, from column w/2: isolated 2 x 2 blocks on a lattice of period 4, the one at lattice position
    (1, 1) grown to 3 x 3.  Returns (mask, n_components, area, area_largest, second largest); the same under 4- and 8-connectivity."""
    assert h % 4 == 0 and w % 8 == 0 and w >= 32 and h >= 12
    m = np.zeros((h, w), bool)
    ws = w // 2 - 1
    m[:, :ws] = serpentine(h, ws)
    serp = (h // 2) * ws + h // 2                  # h is even: h / 2 full rows and h / 2 joining pixels
    ni, nj = h // 4, (w // 2) // 4
    for i in range(ni):
        for j in range(nj):
            m[4 * i: 4 * i + 2, w // 2 + 4 * j: w // 2 + 4 * j + 2] = True
    m[4: 7, w // 2 + 4: w // 2 + 7] = True
    return m, 1 + ni * nj, serp + 4 * (ni * nj - 1) + 9, serp, 9
