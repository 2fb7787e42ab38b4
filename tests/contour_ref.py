"""The contour contract restated for the tests (DESIGN §3 "Contours"), independent of wire.mask_contours_host and of the kernels: a serial
edge follower in plain Python.  Every unit edge between a set and an unset (or outside) pixel becomes one directed edge with the foreground
on its right (x to the right, y down: a set pixel's top edge runs +x, its right edge +y, its bottom edge -x, its left edge -y); the follower
walks from edge to edge, takes the right turn where a vertex offers two ways on (a saddle), keeps the vertices where the direction changes,
rotates every loop to its smallest (y, x) corner and sorts the loops by that corner.  Also the helpers of the property tests."""
import numpy as np

STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))          # direction 0 +x, 1 +y, 2 -x, 3 -y; (d + 1) % 4 is the right turn


def contours(mask):
    """(H,W) mask -> list of loops, each a list of (x, y) tuples."""
    m = np.asarray(mask).astype(bool)
    h, w = m.shape

    def pix(r, c):
        return 0 <= r < h and 0 <= c < w and bool(m[r, c])

    edges = set()
    for r in range(h):
        for c in range(w):
            if not m[r, c]:
                continue
            if not pix(r - 1, c):
                edges.add((c, r, 0))
            if not pix(r, c + 1):
                edges.add((c + 1, r, 1))
            if not pix(r + 1, c):
                edges.add((c + 1, r + 1, 2))
            if not pix(r, c - 1):
                edges.add((c, r + 1, 3))
    unused = set(edges)
    loops = []
    while unused:
        start = next(iter(unused))
        path, cur = [], start
        while True:
            unused.remove(cur)
            path.append(cur)
            x, y, d = cur
            nx, ny = x + STEP[d][0], y + STEP[d][1]
            nxt = [(nx, ny, nd) for nd in ((d + 1) % 4, d, (d + 3) % 4) if (nx, ny, nd) in edges][0]
            if nxt == start:
                break
            assert nxt in unused, "an edge was reached twice"
            cur = nxt
        verts = [(x, y) for k, (x, y, d) in enumerate(path) if path[k - 1][2] != d]
        k = min(range(len(verts)), key=lambda i: (verts[i][1], verts[i][0]))
        loops.append(verts[k:] + verts[:k])
    loops.sort(key=lambda lp: (lp[0][1], lp[0][0]))
    return loops


def checkerboard(side, parity):
    """side x side, pixel (r, c) set iff (r + c) % 2 == parity."""
    ys, xs = np.mgrid[0:side, 0:side]
    return (ys + xs) % 2 == parity


def unit_squares(mask):
    """Built, not traced: the contours of a mask whose set pixels touch only diagonally (a checkerboard, single pixels), where the right
    turn at every saddle closes one unit square per set pixel, in row-major order of the pixels.  -> (pixels, 4, 2) int32 of (x, y)."""
    ys, xs = np.nonzero(np.asarray(mask).astype(bool))                # row-major
    return np.stack([np.stack([xs, ys], 1), np.stack([xs + 1, ys], 1), np.stack([xs + 1, ys + 1], 1), np.stack([xs, ys + 1], 1)], 1).astype(np.int32)


def as_lists(loops):
    """Loops as (k,2) arrays or lists of pairs -> lists of (x, y) int tuples, for comparison with contours()."""
    return [[(int(x), int(y)) for x, y in np.asarray(lp).reshape(-1, 2)] for lp in loops]


def area2(loop):
    """sum(x_i * y_{i+1} - x_{i+1} * y_i) over the closed loop, in Python integers."""
    n = len(loop)
    return sum(int(loop[i][0]) * int(loop[(i + 1) % n][1]) - int(loop[(i + 1) % n][0]) * int(loop[i][1]) for i in range(n))


def fill_even_odd(loops, h, w):
    """Even-odd fill of a list of loops: pixel (r, c) is set iff an odd number of vertical loop edges cross its row to its left."""
    out = np.zeros((h, w), dtype=bool)
    for lp in loops:
        n = len(lp)
        for i in range(n):
            (x0, y0), (x1, y1) = lp[i], lp[(i + 1) % n]
            if x0 == x1 and y0 != y1:
                out[min(y0, y1):max(y0, y1), x0:] ^= True
    return out


def fill_holes(mask):
    """The mask with its holes filled: every unset pixel the frame does not reach through unset pixels with 8 neighbours becomes set."""
    m = np.asarray(mask).astype(bool)
    h, w = m.shape
    p = np.zeros((h + 2, w + 2), dtype=bool)
    p[1:-1, 1:-1] = m
    seen = np.zeros_like(p)
    seen[0, 0] = True
    stack = [(0, 0)]
    while stack:
        r, c = stack.pop()
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                rr, cc = r + dr, c + dc
                if 0 <= rr < h + 2 and 0 <= cc < w + 2 and not p[rr, cc] and not seen[rr, cc]:
                    seen[rr, cc] = True
                    stack.append((rr, cc))
    return ~seen[1:-1, 1:-1]


def blob_mask(rng, h, w):
    """A few seeded discs and rectangles, some cut out again: connected pieces with holes and straight and stepped edges."""
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), dtype=bool)
    for k in range(rng.randint(1, 5)):
        cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1, h / 2 + 1), rng.uniform(1, w / 2 + 1)
        shape = ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1 if rng.rand() < 0.6 else (abs(ys - cy) <= ry / 2) & (abs(xs - cx) <= rx / 2)
        m = m & ~shape if (k and rng.rand() < 0.3) else m | shape
    return m


def random_masks(seed, count, lo, hi):
    """`count` seeded masks of lo..hi x lo..hi, alternately blobs and noise of density 0.2 .. 0.8."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        h, w = rng.randint(lo, hi + 1), rng.randint(lo, hi + 1)
        out.append(blob_mask(rng, h, w) if i % 2 == 0 else rng.rand(h, w) < rng.uniform(0.2, 0.8))
    return out
