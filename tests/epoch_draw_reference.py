"""The stated function of dg_epoch_draw (include/depthg_corr.h), restated in plain Python integers: one Philox4x32-10 word and the three
lines of a slot.  tests/test_epoch_cpu.py holds ops.epoch_draw's CPU route against it, tests/test_gpu_epoch_draw.py the kernel."""
import torch

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


def philox_word0(seed, counter):
    """Word 0 of Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3") with the 64-bit key `seed` at the 128-bit
    counter (counter, 0)."""
    c0, c1, c2, c3 = counter & M32, (counter >> 32) & M32, 0, 0
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0


def epoch_draw(state, order, nns, B, num_neighbors):
    """(ind, ind_pos, state after) of one call, all as lists of Python ints.  state: [seed, draws, cursor] as the int64 words hold them."""
    seed, draws, cursor = (int(v) & M64 for v in state)
    order, nns = [int(v) for v in order], [[int(v) for v in row] for row in nns]
    n = len(order)
    ind, ind_pos = [], []
    for j in range(B):
        i = order[min((cursor + j) & M64, n - 1)]                # ind = order[cursor + j], the position held inside the buffer
        r = 1 + philox_word0(seed, (draws + j) & M64) % num_neighbors
        ind.append(i)
        ind_pos.append(nns[min(max(i, 0), n - 1)][r])
    signed = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    return ind, ind_pos, [signed(seed), signed((draws + B) & M64), signed((cursor + B) & M64)]


def case(n_images, K, seed=0):
    """A shuffled order and a table whose column 0 is the image itself and whose other entries are random images."""
    g = torch.Generator().manual_seed(seed + 1000 * n_images + K)
    order = torch.randperm(n_images, generator=g)
    nns = torch.randint(0, n_images, (n_images, K), generator=g)
    nns[:, 0] = torch.arange(n_images)
    return order, nns
