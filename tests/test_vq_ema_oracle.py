"""Pin of oracle/vq_oracle.codebook_ema_update against the UNMODIFIED upstream CosineSimCodebook in training mode: its inputs and
results, recorded by tests/golden/make_golden_upstream_pins.py, are in tests/golden/upstream_pins.npz.  CPU."""
import os

import numpy as np
import torch

from oracle import vq_oracle as V
from tests.golden.cases import CODEBOOK_EMA_CASES, codebook_ema_inputs

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upstream_pins.npz")


def test_codebook_ema_update_matches_upstream():
    """upstream's training-mode forward on the inputs of cases.codebook_ema_inputs, after torch.manual_seed(123)."""
    pins = np.load(PINS)
    for K, R, thr in CODEBOOK_EMA_CASES:
        e0, c0, z = codebook_ema_inputs(K, R)
        ind, embed, cluster = (torch.from_numpy(pins[f"codebook_ema.{K}.{k}"]) for k in ("ind", "embed", "cluster"))
        ind = ind.long()
        ind_o, _ = V.assign_codes(z.reshape(-1, 32), e0)
        assert torch.equal(ind.reshape(-1), ind_o)
        # the oracle's dead-code rows: what sample_vectors draws with the same seed (randperm is the first RNG use of the forward)
        e1, c1 = V.codebook_ema_update(e0, c0, z, ind, 0.9)
        rows = None
        if thr > 0:
            dead = c1 < thr
            n = int(dead.sum())
            if n:
                torch.manual_seed(123)
                Rr = z.reshape(-1, 32).shape[0]
                idx = torch.randperm(Rr)[:n] if Rr >= n else torch.randint(0, Rr, (n,))
                rows = torch.nn.functional.normalize(z.reshape(-1, 32)[idx], dim=-1)
        e1, c1 = V.codebook_ema_update(e0, c0, z, ind, 0.9, threshold_dead=thr, replace_rows=rows)
        assert torch.allclose(c1, cluster, rtol=1e-6, atol=1e-7), (K, (c1 - cluster).abs().max())
        assert torch.allclose(e1, embed, rtol=1e-5, atol=1e-7), (K, (e1 - embed).abs().max())
