"""The class-token tail: ViT's last encoder layer computed for row 0 only (csrc/cls_tail.hip, EncoderLayer.forward_first_row).

CPU part: the algebra in fp64.  GPU part: the two kernels against fp64 attention and against the error of the path they replace,
ViT with the tail against the oracle and against the full last layer, the bit-exact properties, and the fallbacks.

Kernel-error bound (test_kernels_against_fp64_and_the_present_path).  The reference is fp64 attention for one query per image
and head, computed from the SAME bf16 x, q and gamma-folded bf16 weights (what `_fold_ln` makes and the chained encoder's QKV
GEMM consumes).  The path the kernels replace - rows normalised to bf16, ops.linear for K and V, ops.attention with Lq = 1 - has
three bf16 rounding points between x and o (normalised rows / K and V / o; the softmax weights are rounded to bf16 for the MFMA
in both paths); the new path has four of the same size (u / ctx / o, and the weights carry rstd).  Independent roundings of
equal size add in squares, sqrt(4 / 3) = 1.15; the bound is 1.5 x the present path's rel-L2 on the same inputs.
"""
import math

import pytest
import torch

torch.set_grad_enabled(False)
gpu = pytest.mark.gpu

REL_L2, MAX_ABS = 2e-2, 8e-2  # tests/test_hip_vit.py


# ---------------------------------------------------------------- CPU: the algebra
def _ln64(x, g, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b, mean.squeeze(-1), (1.0 / torch.sqrt(var + eps)).squeeze(-1)


def test_algebra_equals_attention_on_token_0_fp64():
    """u_h = W'k,h^T q_h scores the stored rows, ctx_h sums the normalised rows, o_h = W'v,h ctx_h + c_v,h: equal to ordinary
    attention's row 0, with the k side's constant dropped (softmax is shift-invariant).  Both context forms."""
    g = torch.Generator().manual_seed(5)
    N, L, d, H, hd, eps = 3, 23, 32, 2, 16, 1e-6
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x = r(N, L, d) * (0.5 + torch.rand(N, L, 1, generator=g, dtype=torch.float64)) + 2.0 * r(N, L, 1)
    gam, bet = 1.0 + 0.3 * r(d), 0.2 * r(d)
    wq, wk, wv = r(H * hd, d) / math.sqrt(d), r(H * hd, d) / math.sqrt(d), r(H * hd, d) / math.sqrt(d)
    bq, bk, bv = 0.1 * r(H * hd), 0.1 * r(H * hd), 0.1 * r(H * hd)
    xn, mean, rstd = _ln64(x, gam, bet, eps)
    # ordinary attention, row 0
    q = (xn[:, 0] @ wq.T + bq).view(N, H, hd)
    k = (xn @ wk.T + bk).view(N, L, H, hd)
    v = (xn @ wv.T + bv).view(N, L, H, hd)
    p = torch.softmax(torch.einsum("nhe,nlhe->nhl", q, k) / math.sqrt(hd), -1)
    want = torch.einsum("nhl,nlhe->nhe", p, v)
    # the tail
    wkf, wvf = (wk * gam).view(H, hd, d), (wv * gam).view(H, hd, d)
    cv = (wv @ bet + bv).view(H, hd)
    u = torch.einsum("nhe,hed->nhd", q, wkf)
    s = rstd[:, None, :] * (torch.einsum("nhd,nld->nhl", u, x) - mean[:, None, :] * u.sum(-1, keepdim=True)) / math.sqrt(hd)
    p2 = torch.softmax(s, -1)
    ctx = torch.einsum("nhl,nld->nhd", p2, (x - mean[..., None]) * rstd[..., None])
    w = p2 * rstd[:, None, :]
    ctx_raw = torch.einsum("nhl,nld->nhd", w, x) - (w * mean[:, None, :]).sum(-1, keepdim=True)
    for c in (ctx, ctx_raw):
        got = torch.einsum("nhd,hed->nhe", c, wvf) + cv
        assert (got - want).abs().max().item() <= 1e-10


# ---------------------------------------------------------------- GPU: the kernels
def _kernel_case(L, d, H, seed):
    """bf16 x with per-row scale and offset (|mean| / std up to 4), q, folded weights; fp64 reference o (N, H*64)."""
    g = torch.Generator().manual_seed(seed)
    N, hd, eps = 3, 64, 1e-6
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    std = 0.25 + 1.5 * torch.rand(N, L, 1, generator=g)
    ratio = 8.0 * torch.rand(N, L, 1, generator=g) - 4.0  # mean / std of a row, uniform in [-4, 4]
    ratio[:, ::7] = 4.0
    x = ((r(N, L, d) + ratio) * std).to(torch.bfloat16)
    q = r(N, H * hd).to(torch.bfloat16)
    wk = (r(H * hd, d) / math.sqrt(d) * (1.0 + 0.2 * r(d))).to(torch.bfloat16)  # gamma folded in
    wv = (r(H * hd, d) / math.sqrt(d) * (1.0 + 0.2 * r(d))).to(torch.bfloat16)
    ck, cv = 0.1 * r(H * hd), 0.1 * r(H * hd)
    x64 = x.double()
    mean = x64.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x64 - mean) ** 2).mean(-1, keepdim=True) + eps)
    xn = (x64 - mean) * rstd
    k = (xn @ wk.double().T + ck.double()).view(N, L, H, hd)
    v = (xn @ wv.double().T + cv.double()).view(N, L, H, hd)
    p = torch.softmax(torch.einsum("nhe,nlhe->nhl", q.double().view(N, H, hd), k) / math.sqrt(hd), -1)
    want = torch.einsum("nhl,nlhe->nhe", p, v).reshape(N, H * hd)
    stats = torch.cat([mean, rstd], -1).float().view(N * L, 2)
    return dict(x=x, q=q, wk=wk, wv=wv, ck=ck, cv=cv, stats=stats, want=want, eps=eps)


def _rel(got, want):
    return ((got.double().cpu() - want).norm() / want.norm()).item()


KERNEL_CASES = [(50, 192, 3), (197, 768, 12), (577, 1024, 16), (1370, 192, 3), (1370, 768, 12), (197, 1024, 16), (50, 768, 16)]


@gpu
@pytest.mark.parametrize("L,d,H", KERNEL_CASES)
def test_kernels_against_fp64_and_the_present_path(L, d, H):
    from pytorch_models._hip import ops

    c = _kernel_case(L, d, H, 100 + L + d + H)
    N, hd = 3, 64
    x, q, wk, wv = (c[n].cuda() for n in ("x", "q", "wk", "wv"))
    ck, cv, stats = c["ck"].cuda(), c["cv"].cuda(), c["stats"].cuda()
    # the path the kernels replace: normalised rows, K / V projection, attention with one query
    xn = ops.layernorm(x.view(N * L, d), None, None, c["eps"])
    kv = ops.linear(xn, torch.cat([wk, wv]).contiguous(), torch.cat([ck, cv]).contiguous()).view(N, L, 2 * H * hd)
    present = ops.attention(q.view(N, 1, H * hd), kv[..., : H * hd], kv[..., H * hd :], H).view(N, H * hd)
    e_present = _rel(present, c["want"])
    wku = wk.view(H, hd, d).transpose(1, 2).contiguous()
    wvh = wv.view(H, hd, d).contiguous()
    for given in (True, False):
        u = ops.cls_head_gemm(q, wku)
        ctx = ops.cls_attend(x, stats if given else None, u, hd ** -0.5, c["eps"])
        o = ops.cls_head_gemm(ctx, wvh, cv).view(N, H * hd)
        e_new = _rel(o, c["want"])
        print(f"cls_tail kernels L={L} d={d} H={H} stats={'given' if given else 'in-kernel'}: rel-L2 new {e_new:.3e}  present {e_present:.3e}"
              f"  ratio {e_new / e_present:.2f}")
        assert torch.isfinite(o.float()).all()
        assert e_new <= 1.5 * e_present, (L, d, H, given, e_new, e_present)
        # a strided view of a larger tensor (the encoder passes row / batch strides) and a different batch: the same bits
        big = torch.zeros(N + 1, L + 3, d, dtype=torch.bfloat16, device="cuda")
        big[1:, :L] = x
        ctx2 = ops.cls_attend(big[1:, :L], stats if given else None, u, hd ** -0.5, c["eps"])
        assert torch.equal(ctx2, ctx)
        ctx1 = ops.cls_attend(x[1:2], stats[L : 2 * L] if given else None, u[1:2], hd ** -0.5, c["eps"])
        assert torch.equal(ctx1, ctx[1:2])


@gpu
def test_head_gemm_rows_do_not_depend_on_m():
    from pytorch_models._hip import ops

    g = torch.Generator().manual_seed(9)
    x = torch.randn(37, 3 * 64, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(3, 192, 64, generator=g) / 8).to(torch.bfloat16).cuda()
    b = torch.randn(3 * 192, generator=g).cuda()
    y = ops.cls_head_gemm(x, w, b)
    want = torch.einsum("mgk,gnk->mgn", x.double().view(37, 3, 64), w.double()) + b.double().view(3, 192)
    assert ((y.double() - want).norm() / want.norm()).item() < 4e-3  # one bf16 rounding of the result
    assert torch.equal(ops.cls_head_gemm(x[5:6], w, b), y[5:6]) and torch.equal(ops.cls_head_gemm(x[16:], w, b), y[16:])


# ---------------------------------------------------------------- GPU: ViT with the tail
def _build(tag_fn, seed, **kw):
    from pytorch_models.image import ViT
    from synthweights import bf16_round_, fill_module

    m = tag_fn(ViT, **kw).eval()
    fill_module(m, seed)
    bf16_round_(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to(torch.bfloat16).cuda(), sd


def _check(got, want):
    got, want = got.float().cpu(), want.float()
    rel = ((got - want).norm() / want.norm()).item()
    mx = (got - want).abs().max().item()
    assert rel <= REL_L2 and mx <= MAX_ABS, (rel, mx)
    return rel, mx


def _launches(fn):
    """(result, launches of pm_cls_attend while fn ran)"""
    from pytorch_models._hip import ops

    ops.LAUNCH_LOG = {}
    try:
        out = fn()
        n = len(ops.LAUNCH_LOG.get("cls_attend", []))
    finally:
        ops.LAUNCH_LOG = None
    return out, n


@gpu
@pytest.mark.parametrize("tag,seed,batch,name", [("B/16", 32, 4, "vit_b"), ("Ti/16", 31, 2, "vit_ti")])
def test_vit_with_the_tail_against_the_oracle_and_the_full_layer(tag, seed, batch, name, monkeypatch):
    from oracle import ref_vit as RV
    from synthweights import synth_input

    m, sd = _build(lambda V: V.from_google(tag), seed)
    x = synth_input(name, (batch, 3, 224, 224), seed)
    monkeypatch.delenv("PM_VIT_CLS_TAIL", raising=False)
    on, n_on = _launches(lambda: m(x.cuda()))
    assert n_on == 1, "the class-token tail did not run"
    rel, mx = _check(on, RV.forward(sd, RV.geometry_from_google(tag), x))
    monkeypatch.setenv("PM_VIT_CLS_TAIL", "0")
    off, n_off = _launches(lambda: m(x.cuda()))
    assert n_off == 0
    d = ((on.float() - off.float()).norm() / off.float().norm()).item()
    print(f"ViT-{tag} batch {batch}: tail vs oracle rel-L2 {rel:.3e} max-abs {mx:.3e}; tail on vs off rel-L2 {d:.3e}")
    assert d <= 1e-2


@gpu
def test_tail_batch_4_is_the_stack_of_batch_1(monkeypatch):
    from synthweights import synth_input

    monkeypatch.delenv("PM_VIT_CLS_TAIL", raising=False)
    m, _ = _build(lambda V: V.from_google("B/16"), 32)
    xb = synth_input("vit_b", (4, 3, 224, 224), 32).cuda()
    got = m(xb)
    assert torch.equal(got, torch.cat([m(xb[i : i + 1]) for i in range(4)]))


@gpu
def test_tail_batch_256_bit_exact_properties(monkeypatch):
    """Batch 256 (two streams, LayerNorms folded, statistics from the chain): permuting the batch permutes the rows, a rerun is
    identical, one stream equals two, a captured graph replays to the same bits; rows 0..3 agree with the batch-4 run."""
    from pytorch_models import transformer as tf
    from pytorch_models.graph import GraphedForward
    from synthweights import synth_input

    monkeypatch.delenv("PM_VIT_CLS_TAIL", raising=False)
    m, _ = _build(lambda V: V.from_google("B/16"), 32)
    big = synth_input("vit_b256", (256, 3, 224, 224), 77).cuda()
    xb4 = synth_input("vit_b", (4, 3, 224, 224), 32).cuda()
    big[:4] = xb4
    out, n = _launches(lambda: m(big))
    assert n == 2 and out.shape == (256, 768) and torch.isfinite(out.float()).all()
    small = m(xb4).float()
    assert ((out[:4].float() - small).norm() / small.norm()).item() < 1e-2
    assert torch.equal(m(big), out)
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(m(big[perm]), out[perm])
    tf.ENCODER_STREAMS = 1
    try:
        one, n1 = _launches(lambda: m(big))
    finally:
        tf.ENCODER_STREAMS = 0
    assert n1 == 1 and torch.equal(one, out)
    g = GraphedForward(m, big)
    assert torch.equal(g(big), out)
    assert torch.equal(g(big[perm]), out[perm])
    monkeypatch.setenv("PM_VIT_CLS_TAIL", "0")
    off = m(big).float()
    d = ((out.float() - off).norm() / off.norm()).item()
    print(f"ViT-B/16 batch 256: tail on vs off rel-L2 {d:.3e}")
    assert d <= 1e-2


# ---------------------------------------------------------------- GPU: the fallbacks
def _on_off(m, x, monkeypatch):
    monkeypatch.delenv("PM_VIT_CLS_TAIL", raising=False)
    on, n = _launches(lambda: m(x))
    monkeypatch.setenv("PM_VIT_CLS_TAIL", "0")
    off = m(x)
    assert n == 0, "the tail ran where the full layer must"
    assert torch.equal(on, off)


@gpu
def test_fallbacks_are_bit_identical_to_the_switch_off(monkeypatch):
    from pytorch_models.image import ViT
    from pytorch_models.transformer import MHA
    from synthweights import bf16_round_, fill_module, synth_input

    x = synth_input("vit_ti", (2, 3, 224, 224), 31).cuda()
    # the gap pooler reads every row
    m = ViT(2, 128, 2, 16, img_size=64, pool_type="gap").eval()
    fill_module(m, 36)
    _on_off(m.to(torch.bfloat16).cuda(), synth_input("vit_gap", (2, 3, 64, 64), 36).cuda(), monkeypatch)
    # siglip: no class token, MAP head
    m, _ = _build(lambda V: V.from_google("Ti/16_siglip"), 33)
    _on_off(m, x, monkeypatch)
    # fp32 parameters
    m = ViT.from_google("Ti/16").eval()
    fill_module(m, 31)
    bf16_round_(m)
    _on_off(m.cuda(), x, monkeypatch)
    # head_dim != 64
    m = ViT(2, 128, 4, 16, img_size=64).eval()
    fill_module(m, 37)
    _on_off(m.to(torch.bfloat16).cuda(), synth_input("vit_gap", (2, 3, 64, 64), 36).cuda(), monkeypatch)

    # a subclassed MHA in the last layer
    class MyMHA(MHA):
        def forward(self, q, k=None, v=None, attn_bias=None, causal=False):
            return MHA.forward(self, q, k, v, attn_bias, causal)

    m, _ = _build(lambda V: V.from_google("Ti/16"), 31)
    m.layers[-1].sa.__class__ = MyMHA
    _on_off(m, x, monkeypatch)
