"""``reference.select_threshold``, the keep rule of top-k then top-p sampling
as one value threshold per row, against the filters of
``reference.sample_token``."""

import pytest
import torch

from trlx_amd.ops import reference


@pytest.mark.parametrize("top_p", [1.0, 0.9, 1e-6])
@pytest.mark.parametrize("top_k", [1, 20, 257, 262])
def test_select_threshold_matches_reference_filters(top_k, top_p):
    V = 257
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(3, V, generator=g) * 3  # tie-free
    assert all(r.unique().numel() == V for r in logits)
    # the kept set of reference.sample_token's filters, written out as there
    lg = logits.clone()
    if 0 < top_k < V:
        kth = torch.topk(lg, top_k, dim=-1).values[..., -1, None]
        lg = lg.masked_fill(lg < kth, float("-inf"))
    if top_p < 1.0:
        sorted_logits, sorted_idx = torch.sort(lg, descending=True, dim=-1)
        probs = torch.softmax(sorted_logits, dim=-1)
        remove = probs.cumsum(dim=-1) - probs > top_p
        sorted_logits = sorted_logits.masked_fill(remove, float("-inf"))
        lg = torch.full_like(lg, float("-inf")).scatter(-1, sorted_idx, sorted_logits)
    thr = reference.select_threshold(logits, top_k, top_p)
    assert torch.equal(logits >= thr[:, None], lg > float("-inf"))


def test_select_threshold_ties_masks_and_inactive_filters():
    ninf = float("-inf")
    s = torch.tensor([[1.0, 1.0, 0.5, ninf, 0.5, -2.0],   # ties are kept together
                      [ninf, 3.0, ninf, ninf, -1.0, ninf],  # fewer than k finite scores
                      [ninf] * 6])                           # nothing to keep
    assert reference.select_threshold(s, 3, 1.0).tolist() == [0.5, -1.0, ninf]
    # top-p over the top-k survivors: row 0's two maxima hold 2 / (2 + 2 e^-0.5) = 0.62
    assert reference.select_threshold(s, 4, 0.5).tolist() == [1.0, 3.0, ninf]
    assert reference.select_threshold(s, 4, 0.7).tolist() == [0.5, 3.0, ninf]
    assert reference.select_threshold(s, 0, 1.0).tolist() == [ninf] * 3  # no filter active
