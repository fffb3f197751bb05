"""Plain-torch restatement of one TACC_block step on the operands the C ABI takes (include/vspbfr_hip.h, "Fused TACC_block step"),
a seeded operand generator with a chosen logit spread, and the regime assertions the kernel tests (tests/test_tacc_kernels.py) and
their CPU twin (tests/test_tacc_ref.py) share.  Nothing here touches the GPU; the dtype of every result follows the operands, so the
same function gives the float64 reference and the fp32 evaluation whose distance from it (`e_ref`) sets the tolerance.

    x  = y * rsqrt(mean_tok(y^2) + 1e-8)                    PixelNorm over the 18 tokens
    P  = x @ wcat^T                -> K, V, q2, v2          columns 0, 512, 1024, 1536
    s  = softmax_j( K @ (eQ + tf*wq)^T / sqrt(18) );  h = s @ V
    A  = softmax_rows( (ek + tf*wk)^T @ q2 / sqrt(512) );   t = v2 @ A
    out = LN(h + LN(t)) * (1 + gamma) + beta                eps 1e-5
    out = c1[k]*out + c2[k]*y      when c1/c2 are given
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

NTOK, D = 18, 512


def tfrac(step, t_div):
    """t / t_div as the C entry forms it: one fp32 division (an operand like any other: both evaluations use this value)."""
    return float(np.float32(step) / np.float32(t_div))


def pixelnorm(y):
    return y * torch.rsqrt((y * y).mean(dim=1, keepdim=True) + 1e-8)


def layer_norm(v):
    return F.layer_norm(v, (v.shape[-1],), None, None, 1e-5)


def tacc_block_ref(y, wcat, eQ, ek, wq, wk, gamma, beta, tf, c1=None, c2=None, k=None):
    """y, eQ, ek, gamma, beta: (B, 18, 512); wcat (2048, 512); wq, wk (512,).  Returns a dict: out, and the intermediates the
    per-launch entry points produce (P, s, h, t) plus the two logit tensors (tok_logits (B,18,18) softmaxed over the last axis,
    chan_logits (B,512,512) [row r, column c] softmaxed over r)."""
    B = y.shape[0]
    x = pixelnorm(y)
    P = x @ wcat.t()
    K, V, q2, v2 = P[..., :D], P[..., D:2 * D], P[..., 2 * D:3 * D], P[..., 3 * D:]
    Q = eQ.reshape(B, NTOK, D) + tf * wq
    tok_logits = K @ Q.transpose(1, 2) / math.sqrt(NTOK)
    s = torch.softmax(tok_logits, dim=-1)
    h = s @ V
    k2 = ek.reshape(B, NTOK, D) + tf * wk
    chan_logits = k2.transpose(1, 2) @ q2 / math.sqrt(D)
    A = torch.softmax(chan_logits, dim=1)
    t = v2 @ A
    out = layer_norm(h + layer_norm(t)) * (1 + gamma.reshape(B, NTOK, D)) + beta.reshape(B, NTOK, D)
    if c1 is not None:
        out = c1[k] * out + c2[k] * y
    return {"out": out, "P": P, "s": s, "h": h, "t": t, "tok_logits": tok_logits, "chan_logits": chan_logits}


def ref_pair(ops, step, t_div, c1=None, c2=None, k=None, y=None):
    """(float64 evaluation, fp32 evaluation) of one block on the fp32 operands `ops` at head row `step`."""
    tf = tfrac(step, t_div)
    res = []
    for dt in (torch.float64, torch.float32):
        c = lambda v: None if v is None else v.to(dt)  # noqa: E731
        res.append(tacc_block_ref(c(ops["y"] if y is None else y), c(ops["wcat"]), c(ops["eQ"]), c(ops["ek"]), c(ops["wq"]), c(ops["wk"]),
                                  c(ops["gamma"][step]), c(ops["beta"][step]), tf, c(c1), c(c2), k))
    return res[0], res[1]


def e_ref(r64, r32, key):
    return float((r32[key].double() - r64[key]).abs().max())


def bound(eref, ref64, factor=4.0, rel=2e-6):
    """max|HIP - float64| <= 4 * e_ref + 2e-6 * max|float64|: the factor covers another summation order over 512 products on MFMA and
    device expf / rsqrtf an ulp or two from the host's; the additive term keeps a lucky e_ref from making the bound unreachable."""
    return factor * eref + rel * float(ref64.abs().max())


# ------------------------------------------------------------------------------------------------ operand generator
def make_operands(seed, B, tok_scale, chan_scale, ek_shift=0.0, eq_shift=0.0, y_scale=3.0, head_steps=3, ties=False):
    """Seeded float64 draws, rounded to fp32 ONCE (the references are evaluated on the rounded values).
    tok_scale: on the K rows of wcat and on eQ (token logits ~ 5.3 tok_scale^2);  chan_scale: on the q2 rows of wcat (channel logits
    ~ 0.2 chan_scale);  ek_shift / eq_shift: a constant added to every element of ek / eQ -- it moves all logits of a channel column /
    of a token row by the same amount, which the softmax must cancel;  ties: two identical eQ token rows and two identical ek channels
    (with the same wk entry), scaled by 8 so that the pair is the maximum of many rows / columns."""
    g = torch.Generator().manual_seed(seed)

    def r(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    y = r(B, NTOK, D) * y_scale
    wcat = r(4 * D, D) / math.sqrt(D)
    wcat[:D] *= tok_scale
    wcat[2 * D:3 * D] *= chan_scale
    eQ = r(B, NTOK, D) * tok_scale + eq_shift
    ek = r(B, NTOK, D) + ek_shift
    wq, wk = r(D), r(D)
    gamma = torch.rand(head_steps, B, NTOK, D, generator=g, dtype=torch.float64)
    beta = r(head_steps, B, NTOK, D) * 0.5
    if ties:
        eQ[:, 4] = 8.0 * eQ[:, 4]
        eQ[:, 11] = eQ[:, 4]
        ek[:, :, 77] = 8.0 * ek[:, :, 77]
        ek[:, :, 300] = ek[:, :, 77]
        wk[300] = wk[77]
    ops = {"y": y, "wcat": wcat, "eQ": eQ, "ek": ek, "wq": wq, "wk": wk, "gamma": gamma, "beta": beta}
    return {k: v.float().contiguous() for k, v in ops.items()}


def wcat_fragment_order(wcat):
    """[n / 16][k / 16][lane = 16 (k % 16 / 4) + n % 16][k % 4] (vsp_tacc_block.wcat_frag)."""
    n, k = wcat.shape
    return wcat.view(n // 16, 16, k // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous()


# regime -> generator arguments.  Scales from the spread they give (asserted by check_regime for every generated case).
REGIMES = {
    "flat": dict(tok_scale=0.25, chan_scale=1.0),
    "mid": dict(tok_scale=1.0, chan_scale=4.0),
    "peaked": dict(tok_scale=3.0, chan_scale=130.0),
    "onehot": dict(tok_scale=6.0, chan_scale=400.0),
    "offset": dict(tok_scale=0.25, chan_scale=1.0, ek_shift=1500.0, eq_shift=300.0),
    "ties": dict(tok_scale=1.0, chan_scale=4.0, ties=True),
}
FULL_BATCHES = (1, 2, 3, 5, 8, 16, 17)   # 17: 18 B is a multiple of neither 4 nor 8, and 16 B + ... splits at an odd place
CASES = [(r, b) for r in ("flat", "peaked") for b in FULL_BATCHES] + [(r, b) for r in ("mid", "onehot", "offset", "ties") for b in (1, 3)]
STEP, T_DIV, HEAD_STEPS = 2, 5.4, 3      # tf = 2 / 5.4 = 0.37; the step is not 0, so the heads' step offset and wq / wk are observed


def case_operands(regime, B, salt=0, **over):
    kw = dict(REGIMES[regime])
    kw.update(over)
    return make_operands(1000 * list(REGIMES).index(regime) + 10 * B + salt, B, head_steps=HEAD_STEPS, **kw)


# Several blocks in one call: block i of a case draws its operands with salt 1 + i and reads the previous block's output (block 0: its
# own y).  (regime, B, number of blocks); the regime is asserted on EVERY block along the float64 trajectory.
MULTI_CASES = [("peaked", b, 4) for b in (1, 3, 8, 17)] + [("flat", b, 2) for b in (1, 3)]


def multi_block_operands(regime, B, n_blocks):
    return [case_operands(regime, B, salt=1 + i) for i in range(n_blocks)]


def multi_block_refs(opsl, step, t_div, c1=None, c2=None, k=None):
    """Blocks applied in sequence at head row `step`, then the sampler update on the ORIGINAL y.  Returns (float64 out, fp32 out, the
    float64 pass's per-block dicts of tacc_block_ref)."""
    outs, per_block = [], []
    for dt in (torch.float64, torch.float32):
        y0 = opsl[0]["y"].to(dt)
        cur = y0
        for ops in opsl:
            blk = tacc_block_ref(cur, ops["wcat"].to(dt), ops["eQ"].to(dt), ops["ek"].to(dt), ops["wq"].to(dt), ops["wk"].to(dt),
                                 ops["gamma"][step].to(dt), ops["beta"][step].to(dt), tfrac(step, t_div))
            if dt == torch.float64:
                per_block.append(blk)
            cur = blk["out"]
        if c1 is not None:
            cur = c1.to(dt)[k] * cur + c2.to(dt)[k] * y0
        outs.append(cur)
    return outs[0], outs[1], per_block


def logit_stats(r64):
    tok, chan = r64["tok_logits"], r64["chan_logits"]
    tc = tok - tok.mean(-1, keepdim=True)
    cc = chan - chan.mean(1, keepdim=True)
    top_t = torch.softmax(tok, -1).max(-1).values
    top_c = torch.softmax(chan, 1).max(1).values
    t2 = tok.topk(2, dim=-1).values
    c2 = chan.topk(2, dim=1).values
    return {
        "tok_std": float(tok.std()), "chan_std": float(chan.std()), "tok_max": float(tok.abs().max()), "chan_max": float(chan.abs().max()),
        "tok_cstd": float(tc.std()), "chan_cstd": float(cc.std()),
        "tok_shift": float(tok.mean(-1).abs().median()), "chan_shift": float(chan.mean(1).abs().median()),
        # share of the rows / columns whose common part is beyond expf's fp32 range
        "tok_shifted": float((tok.mean(-1).abs() > 100).double().mean()), "chan_shifted": float((chan.mean(1).abs() > 100).double().mean()),
        "tok_onehot": float((top_t > 0.999).double().mean()), "chan_onehot": float((top_c > 0.99).double().mean()),
        # per sample: rows / columns whose two largest logits coincide
        "tok_ties": (t2[..., 0] - t2[..., 1] <= 1e-12 * t2[..., 0].abs()).sum(-1),
        "chan_ties": (c2[:, 0] - c2[:, 1] <= 1e-12 * c2[:, 0].abs()).sum(-1),
    }


def check_regime(regime, r64, ops=None):
    """Hard assertions on the float64 reference's own logits: a later edit of the generator cannot quietly flatten a case."""
    st = logit_stats(r64)
    msg = f"{regime}: " + ", ".join(f"{k}={v:.3g}" for k, v in st.items() if isinstance(v, float))
    if regime == "flat":
        assert st["tok_std"] < 1 and st["chan_std"] < 0.5, msg
    elif regime == "mid":
        assert 3 <= st["tok_std"] <= 8 and 0.5 <= st["chan_std"] <= 2, msg
    elif regime == "peaked":
        assert st["tok_max"] > 100 and st["chan_max"] > 100, msg
    elif regime == "onehot":   # "most": more than half of the rows / columns
        assert st["tok_onehot"] > 0.5 and st["chan_onehot"] > 0.5, msg
    elif regime == "offset":
        # Flat once the common part is removed.  The common part of token row i is eq_shift * sum_d K[i, d] / sqrt(18), that of channel
        # column c is ek_shift * sum_tok q2[tok, c] / sqrt(512): a constant times a zero-mean sum, so SOME rows / columns necessarily
        # have a small one whatever the constant.  A stated choice, then: more than 100 on at least 60 % of the rows and of the columns.
        assert st["tok_cstd"] < 1 and st["chan_cstd"] < 0.5 and st["tok_shifted"] >= 0.6 and st["chan_shifted"] >= 0.6, msg
    elif regime == "ties":
        if ops is not None:
            assert torch.equal(ops["eQ"][:, 4], ops["eQ"][:, 11]) and torch.equal(ops["ek"][:, :, 77], ops["ek"][:, :, 300])
            assert ops["wk"][77] == ops["wk"][300]
        assert int(st["tok_ties"].min()) >= 2 and int(st["chan_ties"].min()) >= 32, (msg, st["tok_ties"], st["chan_ties"])
    else:
        raise AssertionError(f"unknown regime {regime}")
    return st


# ------------------------------------------------------------------------------------------------ state dict -> operands
def operands_from_state_dict(sd, p, embd, steps, t_div):
    """The C ABI's operands of block `p` (e.g. 'att_mapper.0.') of a Code_diffuser state dict for the condition `embd` (B,18,512):
    what Code_diffuser.prepare_chain computes on the GPU, in the dtype of `sd`.  gamma/beta heads for steps 0..steps-1."""
    wcat = torch.cat([sd[p + "k_matrix.weight"], sd[p + "v_matrix.weight"], sd[p + "attention_layer.q_matrix.weight"],
                      sd[p + "attention_layer.v_matrix.weight"]], 0)
    Wq, Wk = sd[p + "q_matrix.weight"], sd[p + "attention_layer.k_matrix.weight"]

    def head(name, last):
        W0, b0 = sd[f"{p}{name}.0.weight"], sd[f"{p}{name}.0.bias"]
        rows = []
        for s in range(steps):
            g = embd @ W0[:, :D].t() + b0 + tfrac(s, t_div) * W0[:, D]
            g = F.layer_norm(g, (D,), sd[f"{p}{name}.1.weight"], sd[f"{p}{name}.1.bias"], 1e-5)
            g = F.leaky_relu(g, 0.2) * math.sqrt(2)
            rows.append(last(g @ sd[f"{p}{name}.3.weight"].t() + sd[f"{p}{name}.3.bias"]))
        return torch.stack(rows)

    return {"wcat": wcat, "eQ": embd @ Wq[:, :D].t(), "wq": Wq[:, D], "ek": embd @ Wk[:, :D].t(), "wk": Wk[:, D],
            "gamma": head("gamma_", torch.sigmoid), "beta": head("beta_", lambda v: F.leaky_relu(v, 0.2) * math.sqrt(2))}


def scale_attention_weights(sd, tok, chan):
    """A copy of a Code_diffuser state dict whose token-attention q/k matrices are scaled by `tok` and whose channel-attention q/k
    matrices by `chan` (the synthetic weights of oracle/weights.py are flat on purpose)."""
    out = {}
    for k, v in sd.items():
        if k.endswith(("attention_layer.q_matrix.weight", "attention_layer.k_matrix.weight")):
            v = v * chan
        elif k.endswith(("q_matrix.weight", "k_matrix.weight")):
            v = v * tok
        out[k] = v.clone()
    return out
