"""Routings of the tiled-form tests, numpy only.  With TM = moe.TILE_PAIRS the experts' counts are 0, 1, TM - 1, TM, TM + 1 and 2 TM + 1: no tile, one MFMA column, a
tile short of one pair, a whole tile, a second tile of one pair, a third.  (E = 4 has room for 0, 1, TM and 2 TM + 1.)"""
import numpy as np

EK = ((4, 1), (8, 2), (64, 8))


def tiled_ids(E, k, TM):
    """ids [rows][k]: expert 0 gets no pair, 1..5 the counts above, 61 more pairs are dealt over the experts from 6 on; ONE word is out of range; then shuffled, so that
    a list's pairs lie scattered (the pair count is a multiple of k by construction)"""
    counts = {1: 1, 2: TM, 3: 2 * TM + 1} if E == 4 else {1: 1, 2: TM - 1, 3: TM, 4: TM + 1, 5: 2 * TM + 1}
    rest = [] if E == 4 else (6 + np.arange(61) % (E - 6)).tolist()
    flat = np.array([e for e, c in counts.items() for _ in range(c)] + rest + [-3 if k == 1 else E], np.int32)
    assert len(flat) % k == 0
    return np.random.default_rng(E + k).permutation(flat).reshape(-1, k)
