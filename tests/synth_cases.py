"""Shared by the noise-synthesis tests: a numpy Philox4x32-10 and a float64 oracle of the definitions in include/fgc.h
(fgc_synth_noise), written from that text alone."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (values < 2^32) of one shape, key: two ints.  Returns four uint64 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def gaussians(nv, step, seed, stream):
    """z [nv, 4] float64: the four Gaussians of every vertex for (seed, step, stream)."""
    i = np.arange(nv, dtype=np.uint64)
    full = lambda v: np.full(nv, v, dtype=np.uint64)
    x = philox4x32_10((i, full(step & MASK), full((step >> 32) & MASK), full(stream & MASK)), (seed & MASK, seed >> 32))
    u = [((w >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for w in x]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)


def directions(z):
    d = z[:, :3]
    return d / np.sqrt((d * d).sum(1, keepdims=True))


def vertex_normals(V, F):
    """Unit area-weighted vertex normals in float64."""
    V = np.asarray(V, dtype=np.float64)
    F = np.asarray(F).astype(np.int64)
    cp = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    out = np.zeros_like(V)
    for k in range(3):
        np.add.at(out, F[:, k], cp)
    return out / np.sqrt((out * out).sum(1, keepdims=True))


def oracle(V, F, sigma, step, seed, stream, direction="random"):
    """The displaced vertices in float64: V + d sigma z3."""
    V = np.asarray(V, dtype=np.float64)
    z = gaussians(V.shape[0], step, seed, stream)
    d = directions(z) if direction == "random" else vertex_normals(V, F)
    return V + d * (float(sigma) * z[:, 3:4])


def rows_in_node_order(per_face, permutations, n_nodes):
    """[F, c] per-face rows -> [n_nodes, c] in node order, zero rows for the fake nodes (permutations: old -> new)."""
    per_face = np.asarray(per_face)
    padded = np.concatenate([per_face, np.zeros((n_nodes - per_face.shape[0], per_face.shape[1]), per_face.dtype)])
    new_to_old = np.empty(n_nodes, dtype=np.int64)
    new_to_old[np.asarray(permutations)] = np.arange(n_nodes)
    return padded[new_to_old]
