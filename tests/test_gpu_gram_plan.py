"""The panel Gram under every plan its host code can hand it (csrc/gram_plan.h): forced row splits
(OBHIP_GRAM_NSPLIT) and both dealings of the task table to the XCDs (OBHIP_GRAM_CONTINUOUS), paths the
shape-driven choice takes only at sizes no quick test runs.

Two term sets of tests/test_gpu_gram_dedup.py at n = 1500 rows (24 row tiles, so up to 3 splits): the
constructed one (p = 512: four tiles, one complete group of four diagonal tiles, tile pair (0, 3) skipped) and
the single-factor one (p = 380: three tiles, the last padded, no group, nothing skipped).  Per split: G is finite
and exactly symmetric, within the tolerance extended_ref.ref_gram gives a computed entry (none of this file's
own); the two dealings give the same bits (a dealing moves tasks between XCDs and changes no sum); and the
entries of kept tile pairs are the bits of the run with OBHIP_GRAM_DEDUP=0 under the same plan."""
import numpy as np
import pytest

import extended_ref as E
from test_gpu_gram_dedup import fill_table, gram, info, skipped_mask, small_model, small_rows

pytestmark = pytest.mark.gpu

N = 1500


@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("which,skipped", [("constructed", 1), ("single", 0)])
def test_forced_plans(which, skipped, nsplit, monkeypatch):
    from outerbase_amd import obmod
    m, c = small_model(which), small_rows(which, N)
    t = obmod._Terms(m["om_d"], m["terms"])
    assert info(t)[1] == skipped
    kept = ~skipped_mask(fill_table(t))
    assert kept.all() == (skipped == 0)
    monkeypatch.setenv("OBHIP_GRAM_NSPLIT", str(nsplit))
    G = {}
    for dedup in ("1", "0"):
        if dedup == "0":
            monkeypatch.setenv("OBHIP_GRAM_DEDUP", "0")
        for cont in ("0", "1"):
            monkeypatch.setenv("OBHIP_GRAM_CONTINUOUS", cont)
            G[dedup, cont] = gram(m["om_d"], t, c["x"], poison=dedup == "1")
    for key, g in G.items():
        ratio = E.worst_ratio(g[c["cols"], :], c["want"], c["tol"])
        print("%s nsplit %d dedup %s continuous %s: err/tol %.3g" % ((which, nsplit) + key + (ratio,)))
        assert np.all(np.isfinite(g)) and np.array_equal(g, g.T)
        assert ratio <= 1.0
    for dedup in ("1", "0"):
        assert np.array_equal(G[dedup, "0"], G[dedup, "1"]), "the dealing changed a sum"
    for cont in ("0", "1"):
        assert np.array_equal(G["1", cont][kept], G["0", cont][kept]), "a kept entry differs from the switched-off run"
