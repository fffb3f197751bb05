"""The TACC attention kernels (csrc/tacc_chain.hip, csrc/tacc_kernels.h, csrc/tacc.hip) against a float64 restatement of their
contract (tests/tacc_ref.py), on operands whose softmaxes are NOT flat.  The golden chain tests (test_hip_models.py) use weights
built so that both softmaxes are close to uniform and the chain is contractive: a dropped max, a wrong token or batch index or a
lost partial sum barely moves them.  Here ONE block is driven for ONE step with logits of a chosen spread (regimes of
tacc_ref.REGIMES, each asserted from the reference's own logits), every sample of a batch has operands of its own, and

    max|HIP - float64| <= 4 * e_ref + 2e-6 * max|float64|,     e_ref = max|fp32 CPU evaluation - float64| on the same operands

(softmax outputs: 4 * e_ref + 1e-7).  Nothing in the bound comes from the kernels.  Every comparison prints its e_ref, the HIP error
and their ratio (`pytest -s`); profiles/tacc_pr_gputest.log is such a run on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tacc_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(t):
    return t.to(DEV).contiguous()


def close(a, ref64, eref, what, atol=None):
    """Per sample (dim 0) against float64 under the module's bound; prints the figures first."""
    a = a.detach().cpu().double()
    assert a.shape == ref64.shape, (what, a.shape, ref64.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    tol = R.bound(eref, ref64) if atol is None else atol
    errs = (a - ref64).abs().reshape(a.shape[0], -1).max(1).values if a.numel() else torch.zeros(1, dtype=torch.float64)
    err, worst = float(errs.max()), int(errs.argmax())
    print(f"TACC {what}: e_ref={eref:.3e} e_hip={err:.3e} ratio={err / eref if eref else float('nan'):.2f} tol={tol:.3e} "
          f"max|ref|={float(ref64.abs().max()) if ref64.numel() else 0:.3g}")
    assert err <= tol, f"{what}: sample {worst}: max|d|={err:.3e} tol={tol:.3e} (e_ref {eref:.3e})"


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


def gpu_block(ops, frag=False):
    """One vsp_tacc_block of device tensors from host operands (eQ / ek as the [B*18, 512] matrices the ABI names)."""
    blk = {k: dev(ops[k]) for k in ("wcat", "wq", "wk", "gamma", "beta")}
    blk["eQ"] = dev(ops["eQ"].reshape(-1, R.D))
    blk["ek"] = dev(ops["ek"].reshape(-1, R.D))
    if frag:
        blk["wcat_frag"] = dev(R.wcat_fragment_order(ops["wcat"]))
    return blk


def tables(n=7, seed=99):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) * 0.5 + 0.25, torch.rand(n, generator=g) * 0.5 + 0.25


# ------------------------------------------------------------------------------------------------ 1. chain entry, one block, one step
@pytest.mark.parametrize("regime,B", R.CASES)
def test_chain_one_block_one_step(H, regime, B):
    """vsp_tacc_chain_f32 with n_blocks = 1, steps = [2] of 3 prepared head rows (gamma / beta differ per row, so the step * M * D
    offset is observed; tf = 2 / 5.4 so wq / wk matter).  Plain denoiser call with wcat only and with wcat_frag (bit-identical: the
    fragment order changes addresses, not arithmetic), and the sampler update c1[k] f(y) + c2[k] y with k = coef_idx != step."""
    ops = R.case_operands(regime, B)
    r64, r32 = R.ref_pair(ops, R.STEP, R.T_DIV)
    R.check_regime(regime, r64, ops)
    plain = H.tacc_chain(dev(ops["y"]), [gpu_block(ops)], [R.STEP], t_div=R.T_DIV)
    close(plain, r64["out"], R.e_ref(r64, r32, "out"), f"chain1 plain {regime} B={B}")
    fragd = H.tacc_chain(dev(ops["y"]), [gpu_block(ops, frag=True)], [R.STEP], t_div=R.T_DIV)
    assert torch.equal(plain, fragd), "wcat_frag and wcat must give the same bits"
    c1, c2 = tables()
    m64, m32 = R.ref_pair(ops, R.STEP, R.T_DIV, c1, c2, 5)
    mixed = H.tacc_chain(dev(ops["y"]), [gpu_block(ops, frag=True)], [R.STEP], coef_idx=[5], c1=dev(c1), c2=dev(c2), t_div=R.T_DIV)
    close(mixed, m64["out"], R.e_ref(m64, m32, "out"), f"chain1 mix {regime} B={B}")
    # the other head rows are really other operands: step 1 must give something else
    other = H.tacc_chain(dev(ops["y"]), [gpu_block(ops)], [1], t_div=R.T_DIV)
    o64, o32 = R.ref_pair(ops, 1, R.T_DIV)
    close(other, o64["out"], R.e_ref(o64, o32, "out"), f"chain1 step1 {regime} B={B}")
    assert float((o64["out"] - r64["out"]).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ 2. four blocks, one step
@pytest.mark.parametrize("B", [1, 3, 8, 17])
def test_chain_four_blocks_peaked(H, B):
    """The ping-pong buffers and the in-place last block: four different peaked blocks in one call against four applications of the
    reference (tolerance measured on the four-block reference), without and with the sampler update (which reads the ORIGINAL x after
    three blocks have run)."""
    assert ("peaked", B, 4) in R.MULTI_CASES
    opsl = R.multi_block_operands("peaked", B, 4)
    blocks = [gpu_block(o, frag=bool(i & 1)) for i, o in enumerate(opsl)]
    r64, r32, per_block = R.multi_block_refs(opsl, R.STEP, R.T_DIV)
    for blk in per_block:   # blocks 1..3 read the previous block's output, not y: each is asserted on what it really sees
        R.check_regime("peaked", blk)
    out = H.tacc_chain(dev(opsl[0]["y"]), blocks, [R.STEP], t_div=R.T_DIV)
    close(out, r64, float((r32.double() - r64).abs().max()), f"chain4 plain peaked B={B}")
    c1, c2 = tables()
    m64, m32, _ = R.multi_block_refs(opsl, R.STEP, R.T_DIV, c1, c2, 3)
    out = H.tacc_chain(dev(opsl[0]["y"]), blocks, [R.STEP], coef_idx=[3], c1=dev(c1), c2=dev(c2), t_div=R.T_DIV)
    close(out, m64, float((m32.double() - m64).abs().max()), f"chain4 mix peaked B={B}")


# ------------------------------------------------------------------------------------------------ 3. several steps == single steps
@pytest.mark.parametrize("B", [1, 3])
def test_chain_several_steps_equal_single_steps(H, B):
    """Bit identity only (flat regime, asserted for both blocks at each head row on the case's y; the golden tests own the float64
    bound of a multi-step chain)."""
    assert ("flat", B, 2) in R.MULTI_CASES
    opsl = R.multi_block_operands("flat", B, 2)
    for s in (0, 1, 2):
        for blk in R.multi_block_refs(opsl, s, R.T_DIV)[2]:
            R.check_regime("flat", blk)
    blocks = [gpu_block(o, frag=True) for o in opsl]
    c1, c2 = tables()
    kw = dict(c1=dev(c1), c2=dev(c2), t_div=R.T_DIV)
    steps, idx = [2, 0, 1], [6, 1, 4]
    whole = H.tacc_chain(dev(opsl[0]["y"]), blocks, steps, coef_idx=idx, **kw)
    x = dev(opsl[0]["y"])
    for s, k in zip(steps, idx):
        x = H.tacc_chain(x, blocks, [s], coef_idx=[k], **kw)
    assert torch.equal(whole, x)
    assert torch.isfinite(whole).all()


# ------------------------------------------------------------------------------------------------ 4. per-launch entry points
def gpu_P(H, ops):
    B = ops["y"].shape[0]
    return H.gemm_nt(H.pixelnorm_dim1(dev(ops["y"])).view(B * R.NTOK, R.D), dev(ops["wcat"]))


@pytest.mark.parametrize("regime,B", R.CASES)
def test_scores(H, regime, B):
    ops = R.case_operands(regime, B)
    r64, r32 = R.ref_pair(ops, R.STEP, R.T_DIV)
    R.check_regime(regime, r64, ops)
    tf = R.tfrac(R.STEP, R.T_DIV)
    P = gpu_P(H, ops)
    eref = R.e_ref(r64, r32, "s")
    s = H.tacc_scores(P, dev(ops["eQ"].reshape(-1, R.D)), dev(ops["wq"]), tf, B)
    close(s, r64["s"], eref, f"scores {regime} B={B}", atol=4 * eref + 1e-7)
    assert float((s.sum(-1) - 1).abs().max()) < 1e-5
    # wq as the strided last column of a (512, 513) Linear weight, K at a non-zero offset of a wider buffer
    W = torch.zeros(R.D, R.D + 1)
    W[:, -1] = ops["wq"]
    wide = torch.zeros(B * R.NTOK, 2048 + 64, device=DEV)
    wide[:, 40:40 + R.D] = P[:, :R.D]
    s2 = H.tacc_scores(wide, dev(ops["eQ"].reshape(-1, R.D)), dev(W)[:, -1], tf, B, k_off=40)
    assert torch.equal(s, s2)


@pytest.mark.parametrize("regime,B", R.CASES)
def test_chan_attn(H, regime, B):
    """t = v2 @ softmax_rows(k2^T q2 / sqrt(512)) before its LayerNorm: default layout; P embedded in a wider buffer with other q2 / v2
    offsets; wk as a strided column of a (512, 513) matrix (the non-vectorised staging branch of chan_attn_mfma_body)."""
    ops = R.case_operands(regime, B)
    r64, r32 = R.ref_pair(ops, R.STEP, R.T_DIV)
    R.check_regime(regime, r64, ops)
    tf = R.tfrac(R.STEP, R.T_DIV)
    P = gpu_P(H, ops)
    eref = R.e_ref(r64, r32, "t")
    ek = dev(ops["ek"].reshape(-1, R.D))
    t = H.tacc_chan_attn(P, ek, dev(ops["wk"]), tf, B)
    close(t, r64["t"], eref, f"chan_attn {regime} B={B}")
    wide = torch.full((B * R.NTOK, 2048 + 64), 7.0, device=DEV)
    wide[:, 36:36 + R.D] = P[:, 2 * R.D:3 * R.D]
    wide[:, 1560:1560 + R.D] = P[:, 3 * R.D:]
    t2 = H.tacc_chan_attn(wide, ek, dev(ops["wk"]), tf, B, q2_off=36, v2_off=1560)
    assert torch.equal(t, t2), "the same values at other offsets / another pitch must give the same bits"
    W = torch.zeros(R.D, R.D + 1)
    W[:, -1] = ops["wk"]
    wcol = dev(W)[:, -1]
    assert wcol.stride(0) == R.D + 1
    t3 = H.tacc_chan_attn(P, ek, wcol, tf, B)
    close(t3, r64["t"], eref, f"chan_attn strided wk {regime} B={B}")


@pytest.mark.parametrize("regime,B", R.CASES)
def test_tail(H, regime, B):
    """out and pn = PixelNorm(out) of vsp_tacc_tail_f32 (token attention folded in), given the float64 t rounded to fp32: without and
    with xold / c1 / c2, and with want_pn=False."""
    ops = R.case_operands(regime, B)
    r64, r32 = R.ref_pair(ops, R.STEP, R.T_DIV)
    R.check_regime(regime, r64, ops)
    tf = R.tfrac(R.STEP, R.T_DIV)
    P = gpu_P(H, ops)
    eQ, wq = dev(ops["eQ"].reshape(-1, R.D)), dev(ops["wq"])
    t = dev(r64["t"].float())
    gamma, beta = dev(ops["gamma"][R.STEP]), dev(ops["beta"][R.STEP])
    y, pn = H.tacc_tail(P, eQ, wq, tf, t, gamma, beta, B)
    close(y, r64["out"], R.e_ref(r64, r32, "out"), f"tail {regime} B={B}")
    pn64, pn32 = R.pixelnorm(r64["out"]), R.pixelnorm(r32["out"])
    close(pn, pn64, float((pn32.double() - pn64).abs().max()), f"tail pn {regime} B={B}")
    y2, none = H.tacc_tail(P, eQ, wq, tf, t, gamma, beta, B, want_pn=False)
    assert none is None and torch.equal(y, y2)
    c1, c2 = tables()
    m64, m32 = R.ref_pair(ops, R.STEP, R.T_DIV, c1, c2, 4)
    ym, pnm = H.tacc_tail(P, eQ, wq, tf, t, gamma, beta, B, xold=dev(ops["y"]), c1=dev(c1), c2=dev(c2), idx=4)
    close(ym, m64["out"], R.e_ref(m64, m32, "out"), f"tail mix {regime} B={B}")
    pm64, pm32 = R.pixelnorm(m64["out"]), R.pixelnorm(m32["out"])
    close(pnm, pm64, float((pm32.double() - pm64).abs().max()), f"tail mix pn {regime} B={B}")


def head_pre_ref(e, wcol, ln_w, ln_b, S, t_div):
    rows = [F.leaky_relu(F.layer_norm(e + R.tfrac(s, t_div) * wcol, (R.D,), ln_w, ln_b, 1e-5), 0.2) * np.sqrt(2.0) for s in range(S)]
    return torch.stack(rows)


@pytest.mark.parametrize("S", [1, 4, 50])
@pytest.mark.parametrize("M", [18, 54, 306])
def test_head_pre(H, S, M):
    """lrelu(LN(e + (s / t_div) * wcol) * ln_w + ln_b, 0.2) * sqrt(2) for s = 0..S-1; e carries a common mean of 1e3, where a one-pass
    variance (E[x^2] - E[x]^2) loses everything; wcol contiguous and as the strided last column of a (512, 513) weight."""
    g = torch.Generator().manual_seed(S * 1000 + M)
    e = (torch.randn(M, R.D, generator=g, dtype=torch.float64) + 1e3).float()
    wcol = (torch.randn(R.D, generator=g, dtype=torch.float64) * 3).float()
    ln_w = (torch.rand(R.D, generator=g, dtype=torch.float64) + 0.5).float()
    ln_b = (torch.randn(R.D, generator=g, dtype=torch.float64) * 0.1).float()
    t_div = 50.0
    r64 = head_pre_ref(e.double(), wcol.double(), ln_w.double(), ln_b.double(), S, t_div)
    r32 = head_pre_ref(e, wcol, ln_w, ln_b, S, t_div)
    eref = float((r32.double() - r64).abs().max())
    out = H.tacc_head_pre(dev(e), dev(wcol), dev(ln_w), dev(ln_b), S, t_div).view(S, M, R.D)
    close(out, r64, eref, f"head_pre S={S} M={M}")
    W = torch.zeros(R.D, R.D + 1)
    W[:, -1] = wcol
    out2 = H.tacc_head_pre(dev(e), dev(W)[:, -1], dev(ln_w), dev(ln_b), S, t_div).view(S, M, R.D)
    assert torch.equal(out, out2)


# ------------------------------------------------------------------------------------------------ 5. the three implementations agree
def test_three_implementations_agree_peaked(H):
    """Chain entry, Code_diffuser.chain_step and the per-op Code_diffuser.forward on a network whose q/k matrices are scaled into the
    peaked regime, one denoiser call (four blocks), B = 3, against oracle.models.code_diffuser in float64.  The only test through
    prepare_chain: embed + tacc_head_pre + the head GEMM at non-flat inputs."""
    from oracle import cases, models as OM, weights
    from vspbfr_amd.diffusion import Code_diffuser
    B, T, step = 3, 10, 6
    sd = R.scale_attention_weights(weights.synth_state_dict("diffuser", weights.load_specs()["diffuser"], cases.SEED), 14.0, 12.0)
    g = torch.Generator().manual_seed(17)
    x = (torch.randn(B, 18, 512, generator=g, dtype=torch.float64) * 3).float()
    cond = torch.randn(B, 18, 512, generator=g, dtype=torch.float64).float()
    sd64 = {k: v.double() for k, v in sd.items()}
    ti = torch.full((B,), step, dtype=torch.long)
    r64 = OM.code_diffuser(sd64, x.double(), cond.double(), ti, T)
    r32 = OM.code_diffuser(sd, x, cond, ti, T)
    eref = float((r32.double() - r64).abs().max())
    # every block of this network is peaked on these inputs (asserted along the float64 trajectory)
    cur = x.double()
    for i in range(4):
        o = R.operands_from_state_dict(sd64, f"att_mapper.{i}.", cond.double(), T, T)
        blk = R.tacc_block_ref(cur, o["wcat"], o["eQ"], o["ek"], o["wq"], o["wk"], o["gamma"][step], o["beta"][step], R.tfrac(step, T))
        R.check_regime("peaked", blk)
        cur = blk["out"]
    assert float((cur - r64).abs().max()) <= 1e-9 * float(r64.abs().max())
    net = Code_diffuser(timesteps=T)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    state = net.prepare_chain(dev(cond), T)
    close(H.tacc_chain(dev(x), state, [step], t_div=T), r64, eref, "3impl chain entry")
    got, _ = net.chain_step(dev(x), H.pixelnorm_dim1(dev(x)), state, step)
    close(got, r64, eref, "3impl chain_step")
    close(net(dev(x), dev(cond), ti.to(DEV)), r64, eref, "3impl per-op forward")


# ------------------------------------------------------------------------------------------------ 6. VALU channel attention
def _valu_child():
    """Runs in a fresh interpreter with VSP_TUNE=1 VSP_TACC_VALU=1 (the switch is read once per process): test_chan_attn's default
    case for B = 3, flat and peaked, on the older VALU/LDS kernel.  Prints a checksum of each result for the parent."""
    from vspbfr_amd import hip_ops as Hc
    for regime in ("flat", "peaked"):
        ops = R.case_operands(regime, 3)
        r64, r32 = R.ref_pair(ops, R.STEP, R.T_DIV)
        R.check_regime(regime, r64, ops)
        t = Hc.tacc_chan_attn(gpu_P(Hc, ops), dev(ops["ek"].reshape(-1, R.D)), dev(ops["wk"]), R.tfrac(R.STEP, R.T_DIV), 3)
        close(t, r64["t"], R.e_ref(r64, r32, "t"), f"chan_attn VALU {regime} B=3")
        print(f"CHECKSUM {regime} {float(t.double().sum()):.17g}")


def test_valu_chan_attn_in_child_process(H):
    """The VALU form of the channel attention (kept behind VSP_TUNE=1 VSP_TACC_VALU=1 for A/B runs) passes the same check as the MFMA
    form; its sums run in another order, so a checksum equal to the MFMA form's would mean the switch selected nothing."""
    env = dict(os.environ, VSP_TUNE="1", VSP_TACC_VALU="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "valu-child"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    sums = {ln.split()[1]: ln.split()[2] for ln in p.stdout.splitlines() if ln.startswith("CHECKSUM")}
    assert set(sums) == {"flat", "peaked"}
    same = 0
    for regime in sums:
        ops = R.case_operands(regime, 3)
        t = H.tacc_chan_attn(gpu_P(H, ops), dev(ops["ek"].reshape(-1, R.D)), dev(ops["wk"]), R.tfrac(R.STEP, R.T_DIV), 3)
        same += f"{float(t.double().sum()):.17g}" == sums[regime]
    assert same < 2, "the child computed the MFMA form's bits: the VALU switch was not honoured"


# ------------------------------------------------------------------------------------------------ 7. refusals and empty batches
def chain_params(H, x, blk, work, work_floats, n_tok=18, steps=(0,)):
    from vspbfr_amd._lib import TaccBlock, TaccChainParams
    arr = (TaccBlock * 1)()
    for name in ("wcat", "eQ", "ek", "wq", "wk", "gamma", "beta"):
        setattr(arr[0], name, blk[name].data_ptr())
    p = TaccChainParams()
    p.B, p.n_tok, p.dim, p.n_blocks = x.shape[0], n_tok, 512, 1
    p.blocks = arr
    p.x, p.work, p.work_floats = x.data_ptr(), work.data_ptr(), work_floats
    st = (C.c_int * len(steps))(*steps)
    p.n_steps, p.step = len(steps), st
    p.t_div, p.head_steps = 1.0, 3
    return p, (arr, st)


def test_refusals(H):
    """Argument checks on the host: each raises RuntimeError (or returns an error code from the C entry) and launches nothing -- x
    keeps its bits and the device is still healthy afterwards."""
    B = 2
    ops = R.case_operands("flat", B)
    blk = gpu_block(ops)
    x = dev(ops["y"])
    x0 = x.clone()
    c1, c2 = (dev(t) for t in tables())
    P = gpu_P(H, ops)
    t = torch.zeros(B, 18, 512, device=DEV)
    with pytest.raises(RuntimeError):
        H.tacc_tail(P, blk["eQ"], blk["wq"], 0.3, t, blk["gamma"][0], blk["beta"][0], B, k_off=2)
    with pytest.raises(RuntimeError):
        H.tacc_tail(P, blk["eQ"], blk["wq"], 0.3, t, blk["gamma"][0], blk["beta"][0], B, v_off=514)
    big = torch.zeros(B * 18 * 512 + 4, device=DEV)
    view = big[1:1 + B * 18 * 512].view(B, 18, 512)      # contiguous, 4-byte aligned only
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError):
        H.tacc_chain(view, [blk], [0], t_div=1.0)
    assert not big.any()
    with pytest.raises(RuntimeError):
        H.tacc_chain(x, [blk], [0], c1=c1, t_div=1.0)                     # c1 without c2
    with pytest.raises(RuntimeError):
        H.tacc_chain(x, [blk], [0], c2=c2, t_div=1.0)
    with pytest.raises(RuntimeError):
        H.tacc_chain(x, [blk], [3], t_div=1.0)                            # step outside the 3 prepared head rows
    with pytest.raises(RuntimeError):
        H.tacc_chain(x, [blk], [0, 1, 3], t_div=1.0)                      # a bad LATER step: the good ones before it must not have run
    with pytest.raises(RuntimeError):
        H.tacc_chain(x, [blk], [2, -1], t_div=1.0)
    torch.cuda.synchronize()
    assert torch.equal(x, x0)
    # coefficient index outside the tables (7 entries): by coef_idx, and by the step itself when coef_idx is absent
    for idx in ([7], [-1], [1 << 20]):
        with pytest.raises(RuntimeError):
            H.tacc_chain(x, [blk], [0], coef_idx=idx, c1=c1, c2=c2, t_div=1.0)
    with pytest.raises(RuntimeError):
        H.tacc_chain(x, [blk], [2], c1=c1[:2].contiguous(), c2=c2[:2].contiguous(), t_div=1.0)
    with pytest.raises(RuntimeError):
        H.tacc_chain(x, [blk], [0, 1], coef_idx=[0], c1=c1, c2=c2, t_div=1.0)
    # straight through the C entry: work buffer one float short; 17 tokens
    need = H.lib.vsp_tacc_chain_work_floats(B)
    assert need == B * 18 * 512 * 8
    work = torch.zeros(need, device=DEV)
    p, keep = chain_params(H, x, blk, work, need - 1)
    assert H.lib.vsp_tacc_chain_f32(C.byref(p), H._stream()) != 0
    with pytest.raises(RuntimeError):
        H.check(H.lib.vsp_tacc_chain_f32(C.byref(p), H._stream()), "tacc_chain")
    p, keep = chain_params(H, x, blk, work, need, n_tok=17)
    assert H.lib.vsp_tacc_chain_f32(C.byref(p), H._stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and not work.any()
    # and the same parameters, untouched, do run
    p, keep = chain_params(H, x, blk, work, need)
    assert H.lib.vsp_tacc_chain_f32(C.byref(p), H._stream()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x, x0) and torch.isfinite(x).all()


def test_empty_batch(H):
    """B = 0 returns without a launch for every entry point."""
    e = torch.empty(0, 512, device=DEV)
    wq = torch.zeros(512, device=DEV)
    P = torch.empty(0, 2048, device=DEV)
    assert H.tacc_scores(P, e, wq, 0.3, 0).shape == (0, 18, 18)
    assert H.tacc_chan_attn(P, e, wq, 0.3, 0).shape == (0, 18, 512)
    z = torch.empty(0, 18, 512, device=DEV)
    y, pn = H.tacc_tail(P, e, wq, 0.3, z, z, z, 0)
    assert y.shape == (0, 18, 512) and pn.shape == (0, 18, 512)
    assert H.tacc_head_pre(e, wq, wq, wq, 4, 10.0).shape == (0, 512)
    blk = {"wcat": torch.zeros(2048, 512, device=DEV), "eQ": e, "ek": e, "wq": wq, "wk": wq,
           "gamma": torch.empty(3, 0, 18, 512, device=DEV), "beta": torch.empty(3, 0, 18, 512, device=DEV)}
    assert H.tacc_chain(z, [blk], [1], t_div=2.0).shape == (0, 18, 512)
    torch.cuda.synchronize()


if __name__ == "__main__" and sys.argv[1:] == ["valu-child"]:
    sys.path.insert(0, ROOT)
    _valu_child()
