"""The TDM level pipeline (dfm_user_kernel + dfm_level_kernel) and the fused OTM kernel (dfm_otm_beam_kernel) score a (row, user) pair
through the same device functions (csrc/deepfm.hip.inc: dfm_user_setup, dfm_tile_score), so their scores are equal as BYTES wherever
the two searches meet — not only within the fp32 tolerance every other DeepFM test compares under.

One engine holds the tree, the weights and the 33 users of deepfm_ref.search_case(E, L).  The TDM search is traced on the item ids, the
OTM search on the history codes of the same users, with the same beam: both start from the frontier of level floor(log2 beam), and the
OTM search (a complete tree) scores every child of it, so every row of the TDM trace's first scored level has an OTM twin.  Deeper down
the two beams differ (the TDM tree misses nodes); whatever they share is compared too."""
import numpy as np
import pytest

import deepfm_ref as R
from test_gpu_deepfm import deepfm_engine

pytestmark = pytest.mark.gpu

# (E, L): NCT column tiles of 16, NJ = Ep / 16 feature blocks
CASES = [(16, 10), (128, 15), (16, 32)]        # NCT 1, NJ 1 | NCT 2, NJ 8 | NCT 3, NJ 1
# beam 20: 2 x 16 .. 2 x 20 rows = three 16-row tiles, the last partial, four waves; beam 3: one tile, one wave, a one-wave user set-up
BEAMS = [3, 20]


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(E, L):
        if (E, L) not in made:
            tree, w, _ = R.search_case(E, L)
            made[(E, L)] = deepfm_engine(E, L, tree, w)
        return made[(E, L)]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("E,L", CASES)
@pytest.mark.parametrize("beam", BEAMS)
def test_level_pipeline_and_otm_kernel_same_bits(engines, E, L, beam):
    tree, _, seqs = R.search_case(E, L)
    codes = R.history_codes(tree, seqs)
    assert (codes[1] == -1).all()                                # user 1: all padding
    eng = engines(E, L)
    leaf_level = R.SEARCH_DEPTH                                  # the table of search_case holds the complete tree of depth 9: 1023 rows
    level0 = beam.bit_length() - 1
    _, _, _, tc, ts, tn = eng.tdm_beam_search_trace(seqs, beam, 10, use_mask=False)
    assert "dfm_level_kernel<%d, %d>" % (max(E, 16), (L + 2 + 15) // 16) in eng.last_beam_kernel()
    _, _, _, oc, osc, on = eng.otm_beam_search_trace(codes, beam, leaf_level, leaf_level - level0)
    assert eng.last_beam_kernel() == "dfm_otm_beam_kernel<%d, %d>" % (max(E, 16), (L + 2 + 15) // 16)
    joined = 0
    for u in range(seqs.shape[0]):
        for it in range(min(tn.shape[1], on.shape[1])):
            n_t, n_o = int(tn[u, it]), int(on[u, it])
            otm = {int(c): osc[u, it, i].tobytes() for i, c in enumerate(oc[u, it, :n_o])}
            if it == 0:
                assert n_t > 0 and n_o == 2 << level0, (u, n_t, n_o)
                assert set(tc[u, 0, :n_t].tolist()) <= set(otm), u          # the join holds every first-level row of the TDM trace
            for i in range(n_t):
                c = int(tc[u, it, i])
                if c in otm:
                    joined += 1
                    assert ts[u, it, i].tobytes() == otm[c], (u, level0 + 1 + it, c, float(ts[u, it, i]),
                                                               float(np.frombuffer(otm[c], np.float32)[0]))
    print("E=%d L=%d beam=%d: %d joined (level, code) pairs, all equal as bytes" % (E, L, beam, joined))
    assert joined >= seqs.shape[0]
