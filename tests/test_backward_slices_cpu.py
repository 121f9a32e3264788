"""CPU check of backward._slices, the function that cuts every weight gradient's contraction into slices: whatever (S, chunk) it returns
is what the TN kernels index with, so its invariants are checked over a seeded sweep of the sizes training meets (and beyond)."""
import random


def test_slices_invariants_over_a_seeded_sweep():
    from s2d_amd import backward
    rng = random.Random(20240)
    draws = [(1, 1, 512), (1, 300, 1024), (31, 1, 512), (32, 1, 512), (33, 7, 1024), (511, 9, 512), (512, 9, 512), (513, 9, 1024),
             (4_000_000, 1, 512), (4_000_000, 300, 1024), (942_080, 36, 512), (942_080, 9, 1024), (3_768_320, 4, 1024)]
    for _ in range(50_000):
        # half of the draws log-uniform, so that short contractions are as frequent as long ones
        M = rng.randint(1, 4_000_000) if rng.random() < 0.5 else int(round(10 ** rng.uniform(0, 6.602)))
        draws.append((max(1, min(M, 4_000_000)), rng.randint(1, 300), rng.choice((512, 1024))))
    for M, out_tiles, slots in draws:
        S, chunk = backward._slices(M, out_tiles, slots)
        assert isinstance(S, int) and isinstance(chunk, int), (M, out_tiles, slots)
        assert chunk > 0 and chunk % 32 == 0, (M, out_tiles, slots, S, chunk)          # the kernels' row groups
        assert S * chunk >= M, (M, out_tiles, slots, S, chunk)                          # every row is in a slice
        assert (S - 1) * chunk < M, (M, out_tiles, slots, S, chunk)                     # no empty slice: its partial tile would be read unwritten
        assert 1 <= S <= 65535, (M, out_tiles, slots, S, chunk)                         # gridDim.y
        assert backward._slices(M, out_tiles, slots) == (S, chunk)                      # a function of the arguments alone: a fixed summation order
    assert backward._slices(1000, 4) == backward._slices(1000, 4, 512)                  # the default is the 128-wide tile's slot count
