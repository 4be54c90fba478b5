"""The row walk that phx_influence.hip and phx_knockout.hip share (phx_screen_score.inc), pinned on the MI355X: a
knockout screen laid out as an influence block -- every even call the baseline -- goes through the same walk with the
same W, |u - p| equals |p - u| bit for bit, and the scores come from the same column sums, so the two entry points must
agree in every bit.  Run with `-m gpu`.
"""
import pytest
import torch

from test_influence_gpu import decades

pytestmark = pytest.mark.gpu


# (5, 3, 7, 97): a ragged tail (97 = 24 quads + 1) and several waves; (3, 2, 5, 3): rows too short for a quad
@pytest.mark.parametrize("T,K,B,N", [(5, 3, 7, 97), (3, 2, 5, 3)])
def test_influence_and_knockout_walk_agree_bit_for_bit(T, K, B, N):
    from phoenix_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda:0")
    base = decades((T, B, N), dev, seed=N + K)
    sol = decades((T, K * B, N), dev, seed=N + K + 1)
    g = torch.Generator(device=dev).manual_seed(N)
    sol = torch.where(torch.rand(sol.shape, device=dev, generator=g) < 0.5, sol, -sol)      # signed differences
    genes = [N - 1, 0, N // 2][:K]      # the last and the first column are somebody's gene
    block = torch.stack([base.unsqueeze(1).expand(T, K, B, N), sol.reshape(T, K, B, N)], dim=2)    # [T, K, 2, B, N]
    block = block.reshape(T, 2 * K * B, N).contiguous()
    for k in range(K):
        assert torch.equal(block[:, 2 * k * B:(2 * k + 1) * B], base)
        assert torch.equal(block[:, (2 * k + 1) * B:(2 * k + 2) * B], sol[:, k * B:(k + 1) * B])
    i_scores, targets = engine.influence_scores(block, K, B, genes, want_targets=True)
    k_scores, shift, magnitude = engine.knockout_effects(base, sol, genes, want_matrices=True)
    assert targets.shape == magnitude.shape == (K, N) and bool((magnitude > 0).all())
    assert torch.equal(i_scores, k_scores)
    assert torch.equal(targets, magnitude)
