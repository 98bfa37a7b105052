"""The derived per-element bar of the 16-bit attention kernels (tests/attention_ref.py) holds for the kernels' arithmetic emulated in torch, on every
operand builder at every shape the GPU edge test runs: the bar stays honest if a builder changes.  No device."""

import pytest
import torch

from tests import attention_ref as ar


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ar.BUILDERS)
def test_emulated_kernel_arithmetic_is_inside_the_bound(kind, fmt):
    worst = 0.0
    for B, heads in ar.PAIRS:
        for N in ar.TOKENS:
            x = ar.round_to(ar.build(kind, B, N, heads), fmt)
            ref, S = ar.reference(x)
            bar = ar.bound(S, x[:, :, 2], fmt)
            err = (ar.emulate(x, fmt).double() - ref).abs()
            assert torch.isfinite(err).all()
            ratio = float((err / bar).max())
            assert ratio <= 1.0, f"{kind} {fmt} B={B} heads={heads} N={N}: emulated error / bound = {ratio:.3f}"
            worst = max(worst, ratio)
    print(f"{kind} {fmt}: worst emulated error / bound {worst:.3f}")
    assert worst > 0.05   # a bar twenty times looser than the arithmetic it bounds would see nothing


@pytest.mark.parametrize("N", [1, 63, 64, 65, 319, 385])
def test_planted_operands_name_their_key(N):
    """Every key is the dominant key of one query, and the reference's output row says which: column t(q) mod 64, value 1 + t(q) // 64."""
    x = ar.build("planted", 2, N, 2)
    ref, S = ar.reference(x)
    t = ar.planted_key(N)
    assert sorted(t.tolist()) == list(range(N))
    assert torch.equal(ref.argmax(dim=-1), (t % 64)[None, :, None].expand(2, N, 2))
    want = (1 + t // 64).double()[None, :, None].expand(2, N, 2)
    assert float((ref.amax(dim=-1) - want).abs().max()) < 1e-3   # the other keys together weigh e^-10 or less
    assert torch.equal(ref.abs(), ref) and float((ref - S).abs().max()) == 0.0   # V >= 0: S is the output itself


def test_offset_operands_put_every_real_score_far_below_zero():
    x = ar.round_to(ar.build("offset", 1, 97, 2), "bf16")
    q, k, _ = x.double().permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * 0.125
    assert float(s.max()) < -16.0   # a zero key (score 0) would outweigh all of them together by e^16 / 97
