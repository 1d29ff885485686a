"""numpy restatement of MG_OP_RANDN (csrc/randn.hip), written from the published algorithm and nothing else: Philox4x32-10 of Salmon,
Moraes, Dror and Shaw ("Parallel random numbers: as easy as 1, 2, 3", SC'11) with Random123's constants, uint64 products, and
Box-Muller in float64.  ``check_known_answers`` must pass before anything here judges the kernel
(tests/test_native_noise_host.py::test_restatement_reproduces_the_known_answers, and the fixture of tests/test_gpu_native_noise.py)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # the key increments (golden ratio, sqrt(3) - 1)
MASK32 = 0xFFFFFFFF

# Random123's known-answer vectors for philox4x32, 10 rounds (its kat_vectors file): (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """counter uint32 [..., 4], key uint32 [..., 2] (broadcast against each other) -> uint32 [..., 4]."""
    c = [np.asarray(counter, dtype=np.uint64)[..., k] for k in range(4)]
    k0, k1 = (np.asarray(key, dtype=np.uint64)[..., k] for k in range(2))
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK32), (k1 + np.uint64(W1)) & np.uint64(MASK32)
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]   # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & np.uint64(MASK32), (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & np.uint64(MASK32)]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def check_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = philox4x32_10(np.array(counter), np.array(key))
        assert tuple(int(v) for v in got) == want, (counter, key, [hex(int(v)) for v in got])


def block_words(seed, stream, first_block, n_blocks):
    """uint32 [n_blocks, 4]: blocks first_block ... of stream ``stream`` of ``seed`` (all three: Python ints below 2^64)."""
    blk = np.uint64(first_block) + np.arange(n_blocks, dtype=np.uint64)
    counter = np.stack([blk & np.uint64(MASK32), blk >> np.uint64(32), np.full_like(blk, stream & MASK32), np.full_like(blk, stream >> 32)], axis=-1)
    return philox4x32_10(counter, np.array([seed & MASK32, seed >> 32], dtype=np.uint64))


def _slice(per_block, offset, n):
    return per_block.reshape(-1)[offset % 4: offset % 4 + n]


def _span(offset, n):
    return offset // 4, (offset + n - 1) // 4 - offset // 4 + 1


def words(seed, stream, offset, n):
    """uint32 [n]: the raw words of elements [offset, offset + n) (the op's mode 1)."""
    return _slice(block_words(seed, stream, *_span(offset, n)), offset, n)


def normals(seed, stream, offset, n):
    """float64 [n]: Box-Muller on the same words - words (0, 1) and (2, 3) of a block are pairs (a, b); u = ((a >> 9) + 1) 2^-23,
    v = (b >> 8) 2^-24; r cos(2 pi v), r sin(2 pi v) with r = sqrt(-2 ln u)."""
    w = block_words(seed, stream, *_span(offset, n))
    out = np.empty(w.shape, dtype=np.float64)
    for pair in (0, 2):
        u = ((w[:, pair] >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -23
        v = (w[:, pair + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u))
        out[:, pair], out[:, pair + 1] = r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v)
    return _slice(out, offset, n)
