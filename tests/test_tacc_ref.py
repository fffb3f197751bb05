"""CPU checks of the reference the TACC kernel tests use (tests/tacc_ref.py): the float64 restatement of the C ABI's contract against
oracle.models.tacc_block, and the logit-spread regime of every case the GPU tests generate."""
import pytest
import torch

import tacc_ref as R
from oracle import cases, models as OM, weights

torch.set_grad_enabled(False)


def _sd64(tok=1.0, chan=1.0):
    sd = weights.synth_state_dict("diffuser", weights.load_specs()["diffuser"], cases.SEED)
    return {k: v.double() for k, v in R.scale_attention_weights(sd, tok, chan).items()}


@pytest.mark.parametrize("tok,chan", [(1.0, 1.0), (12.0, 25.0)])
def test_reference_matches_oracle_block(tok, chan):
    """tacc_block_ref on operands derived from a state dict == oracle.models.tacc_block on that state dict, in float64 (flat synthetic
    weights, and the same weights scaled until both softmaxes are far from uniform)."""
    sd = _sd64(tok, chan)
    g = torch.Generator().manual_seed(5)
    B, T, step = 3, 10, 7
    x = torch.randn(B, 18, 512, generator=g, dtype=torch.float64) * 3
    embd = torch.randn(B, 18, 512, generator=g, dtype=torch.float64)
    for p in ("att_mapper.0.", "att_mapper.3."):
        ops = R.operands_from_state_dict(sd, p, embd, T, T)
        tf = R.tfrac(step, T)
        got = R.tacc_block_ref(x, ops["wcat"], ops["eQ"], ops["ek"], ops["wq"], ops["wk"], ops["gamma"][step], ops["beta"][step], tf)
        want = OM.tacc_block(sd, p, x, embd, torch.full((B, 18, 1), tf, dtype=torch.float64))
        assert float((got["out"] - want).abs().max()) <= 1e-11 * float(want.abs().max())
        if tok > 1:
            st = R.logit_stats(got)
            assert st["tok_std"] > 3 and st["chan_std"] > 0.5, st
    # the sampler update on top
    c1, c2 = torch.rand(T, generator=g, dtype=torch.float64), torch.rand(T, generator=g, dtype=torch.float64)
    mixed = R.tacc_block_ref(x, ops["wcat"], ops["eQ"], ops["ek"], ops["wq"], ops["wk"], ops["gamma"][step], ops["beta"][step], tf, c1, c2, 4)
    assert torch.equal(mixed["out"], c1[4] * got["out"] + c2[4] * x)


def test_reference_matches_oracle_denoiser():
    """Four applications of the block reference == oracle.models.code_diffuser (float64)."""
    sd = _sd64()
    g = torch.Generator().manual_seed(6)
    B, T, step = 2, 10, 3
    x = torch.randn(B, 18, 512, generator=g, dtype=torch.float64) * 3
    embd = torch.randn(B, 18, 512, generator=g, dtype=torch.float64)
    cur = x
    for i in range(4):
        ops = R.operands_from_state_dict(sd, f"att_mapper.{i}.", embd, T, T)
        cur = R.tacc_block_ref(cur, ops["wcat"], ops["eQ"], ops["ek"], ops["wq"], ops["wk"], ops["gamma"][step], ops["beta"][step],
                               R.tfrac(step, T))["out"]
    want = OM.code_diffuser(sd, x, embd, torch.full((B,), step, dtype=torch.long), T)
    assert float((cur - want).abs().max()) <= 1e-10 * float(want.abs().max())


@pytest.mark.parametrize("regime,B", R.CASES)
def test_generated_case_is_in_its_regime(regime, B):
    """Every case the GPU tests send lands in the regime it is named after, and one block stays well conditioned there: the fp32
    evaluation is within 2e-4 of float64 on outputs of |max| ~10 (so the 4 * e_ref bound is tight, not a licence).  The offset regime
    is the exception, 3e-3: a common part of several hundred costs the logits their low bits in ANY fp32 evaluation, and with a flat
    channel softmax t is nearly constant along a row, so the LayerNorm over it magnifies what is left."""
    ops = R.case_operands(regime, B)
    r64, r32 = R.ref_pair(ops, R.STEP, R.T_DIV)
    R.check_regime(regime, r64, ops)
    assert torch.isfinite(r32["out"]).all()
    assert R.e_ref(r64, r32, "out") < (3e-3 if regime == "offset" else 2e-4), R.e_ref(r64, r32, "out")
    assert float(ops["y"].abs().max()) > 10


@pytest.mark.parametrize("regime,B,n_blocks", R.MULTI_CASES)
def test_generated_multi_block_case_is_in_its_regime(regime, B, n_blocks):
    """The several-block cases of the GPU tests (operands of their own, blocks after the first reading the previous block's output):
    every block is in the named regime on the input it really sees, at every head row the GPU tests use."""
    opsl = R.multi_block_operands(regime, B, n_blocks)
    for step in ((R.STEP,) if regime == "peaked" else (0, 1, 2)):
        r64, r32, per_block = R.multi_block_refs(opsl, step, R.T_DIV)
        assert len(per_block) == n_blocks
        for blk in per_block:
            R.check_regime(regime, blk)
        assert torch.isfinite(r32).all()


def test_fragment_order_is_a_permutation():
    w = torch.arange(2048 * 512, dtype=torch.float32).view(2048, 512)
    f = R.wcat_fragment_order(w).reshape(-1)
    n, k = 37, 203
    lane = 16 * (k % 16 // 4) + n % 16
    assert f[(((n // 16) * 32 + k // 16) * 64 + lane) * 4 + k % 4] == w[n, k]
    assert torch.equal(f.sort().values, w.reshape(-1))
