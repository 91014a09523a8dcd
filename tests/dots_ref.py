"""The definitions of the exposure masks and the surface dots (include/freesasa_gpu.h, freesasa_amd/csrc/dots_kernels.h) restated
in numpy: the yardstick of tests/test_dots.py and tests/test_dots_gpu.py.  fp64; numpy rounds every elementwise operation on its
own, as the build does with -ffp-contract=off.

    mask       uint32 [n, 4]: bit k & 31 of word k >> 5 of atom i is set iff point k of atom i is exposed; bits k >= N are 0
    dot_first  int64 [n + 1]: the exclusive prefix sum of popcount(mask_i & the N bits that exist)
    dots       atom i ascending, within it exposed k ascending: t = u_k * R_i; t += x_i;  dot_atom = i, dot_point = k
"""
import numpy as np

WORDS = 4  # SR_CAP_WORDS


def full_words(n_points):
    """the bits that exist, word by word: [4] uint32"""
    left = np.clip(n_points - 32 * np.arange(WORDS), 0, 32)
    return np.array([(1 << int(l)) - 1 for l in left], dtype=np.uint32)


def masks_of(exposed):
    """[n, N] bool -> [n, 4] uint32"""
    exposed = np.asarray(exposed, dtype=bool)
    n, N = exposed.shape
    bits = np.zeros((n, 32 * WORDS), dtype=np.uint64)
    bits[:, :N] = exposed
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    return (bits.reshape(n, WORDS, 32) * weights).sum(axis=2).astype(np.uint32)


def bits_of(masks, n_points):
    """[n, 4] uint32 -> [n, N] bool: the bits that exist (stray bits at or above N are ignored)"""
    masks = np.asarray(masks, dtype=np.uint32).reshape(-1, WORDS)
    k = np.arange(n_points)
    return ((masks[:, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)


def popcounts(masks, n_points):
    return bits_of(masks, n_points).sum(axis=1).astype(np.int64)


def dot_first(masks, n_points):
    c = popcounts(masks, n_points)
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(c, dtype=np.int64)])


def dots(xyz, radii, probe, unit, masks):
    """-> (dot_xyz [D, 3] fp64, dot_atom [D] int32, dot_point [D] int32)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    unit = np.asarray(unit, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(radii, dtype=np.float64) + probe
    atom, point = np.nonzero(bits_of(masks, len(unit)))  # (row-major: atoms ascending, points ascending within an atom)
    t = unit[point] * R[atom][:, None]
    t = t + xyz[atom]
    return t, atom.astype(np.int32), point.astype(np.int32)


def random_masks(rng, n, n_points, stray=False):
    """random masks of n atoms, all-zero and all-set atoms among them; stray: bits at and above n_points set at random too"""
    exposed = rng.random((n, n_points)) < rng.random((n, 1))
    kinds = rng.integers(0, 6, n)
    exposed[kinds == 0] = False
    exposed[kinds == 1] = True
    m = masks_of(exposed)
    if stray:
        junk = rng.integers(0, 1 << 32, (n, WORDS), dtype=np.uint64).astype(np.uint32)
        m = m | (junk & ~full_words(n_points))
    return m
