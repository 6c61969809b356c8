"""What the attention test files share (a plain module, imported by them):

* the fp32 oracle of the flash kernels (`heads`, `scores`, `ref`, `rel`) — masked softmax over
  explicitly repeated key/value heads — and `run_case`, the forward / lse / backward comparison
  against it at the suite's bars (o: atol = rtol = 3e-2; lse: atol 2e-2, rtol 1e-3; dq / dk / dv:
  relative L2 error < 2e-2; dead key rows exactly zero);
* the parent-bits cases of tests/test_attention_parent_bits.py: `PARENT_CASES`, `case_inputs`,
  `run_wrappers`, `digests`, and the recorder of tests/golden/attention_parent_bits.json,

      python tests/attention_oracle.py OUT.json COMMIT

  run from a checkout of the commit to record (the package importable, its library built). It uses
  only attention_fwd / attention_bwd / set_fused_attention_bwd / RngState of ops.transformer."""
import hashlib
import json
import math
import os
import sys

import torch

from tensorflow_train_distributed_amd.ops import transformer as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_parent_bits.json")
OUTPUTS = ("o", "lse", "dq", "dk", "dv")


# ------------------------------------------------------------------ fp32 oracle
def heads(t, B, S, Hk, H):
    """[B, H, S, 64] of token-major t [B*S, Hk*64], each key/value head repeated H // Hk times."""
    return t.reshape(B, S, Hk, 64).transpose(1, 2).repeat_interleave(H // Hk, dim=1)


def scores(q, k, B, H, Hk, Sq, Sk, seqlen, causal):
    """[B, H, Sq, Sk] fp32 scores of token-major q [B*Sq, H*64] and k [B*Sk, Hk*64]; masked keys
    at -inf."""
    sc = heads(q, B, Sq, H, H) @ heads(k, B, Sk, Hk, H).transpose(-1, -2) / 8.0
    if seqlen is not None:
        ar = torch.arange(Sk, device=q.device)
        sc = sc.masked_fill(~(ar[None, :] < seqlen[:, None].long())[:, None, None, :], float("-inf"))
    if causal:
        tri = torch.ones(Sq, Sk, dtype=torch.bool, device=q.device).tril()
        sc = sc.masked_fill(~tri, float("-inf"))
    return sc


def ref(q, k, v, B, H, Hk, Sq, Sk, seqlen=None, causal=False, keep=None, p=0.0):
    pr = scores(q, k, B, H, Hk, Sq, Sk, seqlen, causal).softmax(-1)
    if keep is not None:
        pr = pr * keep * T.attention_drop_scale(p)
    return (pr @ heads(v, B, Sk, Hk, H)).transpose(1, 2).reshape(B * Sq, H * 64)


def rel(got, want):
    return float((got.float() - want.float()).norm() / want.float().norm())


def run_case(H, Hk, Sq, Sk, causal, seqlen, p, fused=False, fused_layout=False):
    """Forward, lse and backward of one shape (B = 2) against the oracle. fused_layout: q / k / v and
    dq / dk / dv are column views of one [B*S, (H + 2 Hk)*64] buffer (needs Sq == Sk); otherwise q
    is contiguous and k / v are views of a [B*Sk, 2*Hk*64] buffer, so ldk = ldv != ldq. fused: the
    single-kernel backward switched on for the call."""
    torch.manual_seed(0)
    B = 2
    D, Dk = H * 64, Hk * 64
    dev = "cuda"
    if fused_layout:
        assert Sq == Sk
        qkv = (torch.randn(B * Sq, D + 2 * Dk, device=dev) * 1.5).bfloat16()
        q, k, v = qkv[:, :D], qkv[:, D:D + Dk], qkv[:, D + Dk:]
    else:
        q = (torch.randn(B * Sq, D, device=dev) * 1.5).bfloat16()
        kv = (torch.randn(B * Sk, 2 * Dk, device=dev) * 1.5).bfloat16()
        k, v = kv[:, :Dk], kv[:, Dk:]
    seqlen = torch.tensor(seqlen, dtype=torch.int32, device=dev) if seqlen is not None else None
    rng = T.RngState(99, dev) if p > 0 else None
    if rng is not None:
        rng.advance()
    o = torch.empty(B * Sq, D, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * H, Sq, dtype=torch.float32, device=dev)
    kw = dict(Sk=Sk, Hk=Hk, seqlen=seqlen, p_drop=p, rng=rng, site=5, causal=causal)
    T.attention_fwd(q, k, v, o, lse, B, H, Sq, **kw)
    keep = None
    if p > 0:
        seed, step = rng.host()
        # the host mirror of the absolute-index hash, per query head: H masks, not Hk
        keep = torch.from_numpy(T.attention_keep_mask(seed, step, 5, p, B, H, Sq, Sk)).float().to(dev)
        if causal:  # the triangle zeroes the rest (the -inf mask already does)
            keep = keep * torch.ones(Sq, Sk, device=dev).tril()
    qf, kf, vf = [t.float().requires_grad_(True) for t in (q, k, v)]
    want = ref(qf, kf, vf, B, H, Hk, Sq, Sk, seqlen, causal, keep, p)
    print("o max abs err", float((o.float() - want.detach()).abs().max()))
    torch.testing.assert_close(o.float(), want, atol=3e-2, rtol=3e-2)
    lse_ref = torch.logsumexp(scores(qf, kf, B, H, Hk, Sq, Sk, seqlen, causal), -1).reshape(B * H, Sq) / math.log(2)
    print("lse max abs err", float((lse - lse_ref.detach()).abs().max()))
    torch.testing.assert_close(lse, lse_ref.detach(), atol=2e-2, rtol=1e-3)
    do = torch.randn(B * Sq, D, device=dev).bfloat16()
    want.backward(do.float())
    if fused_layout:
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[:, :D], dqkv[:, D:D + Dk], dqkv[:, D + Dk:]
    else:
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        dk, dv = dkv[:, :Dk], dkv[:, Dk:]
    T.set_fused_attention_bwd(fused)
    try:
        T.attention_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, Sq, **kw)
    finally:
        T.set_fused_attention_bwd(False)
    rels = [(name, rel(got, g)) for name, got, g in (("dq", dq, qf.grad), ("dk", dk, kf.grad), ("dv", dv, vf.grad))]
    print("rel L2", rels)
    for name, r in rels:
        assert r < 2e-2, (name, r)
    if seqlen is not None:  # keys >= len: exact zeros, not small numbers
        dead = (torch.arange(B * Sk, device=dev) % Sk) >= seqlen.long().repeat_interleave(Sk)
        assert bool(dead.any())
        assert float(dk[dead].float().abs().max()) == 0.0 and float(dv[dead].float().abs().max()) == 0.0


# ------------------------------------------------------------------ parent-bits cases
def _cases():
    """id -> (H, Hk, Sq, Sk, seqlen, p, causal, fused): the smallest shapes (B = 2) that reach every
    launched instantiation — two query blocks, a length inside a tile, an odd block count."""
    c = {}
    for name, H, Hk in (("self", 3, 3), ("grouped", 4, 2)):
        for p in (0.0, 0.1):
            for causal in (False, True):
                c["%s-p%g-%s" % (name, p, "causal" if causal else "full")] = (H, Hk, 256, 256, [256, 150], p, causal,
                                                                             False)
    c["grouped-cross-128x384-p0.1"] = (6, 2, 128, 384, [384, 70], 0.1, False, False)
    c["cross-128x384-p0.1"] = (3, 3, 128, 384, [384, 70], 0.1, False, False)
    c["cross-384x128-p0"] = (3, 3, 384, 128, [37, 128], 0.0, False, False)
    for S in (128, 256, 512):
        for p in (0.0, 0.1):
            c["fused-bwd-%d-p%g" % (S, p)] = (3, 3, S, S, [S, S // 2 + 22], p, False, True)
    return c


PARENT_CASES = _cases()
B = 2


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(t.view(torch.int16 if t.dtype == torch.bfloat16 else t.dtype).numpy().tobytes())
    return h.hexdigest()


def case_inputs(cid):
    """(q, k, v, do, seqlen) of a case on the CPU — q / do [B*Sq, H*64], k / v [B*Sk, Hk*64], bf16 of
    randn * 1.5 from a generator seeded by the case's position — and the sha256 of their bytes."""
    H, Hk, Sq, Sk, seqlen, _, _, _ = PARENT_CASES[cid]
    g = torch.Generator().manual_seed(1000 + list(PARENT_CASES).index(cid))
    q, k, v, do = [(torch.randn(B * S, h * 64, generator=g) * 1.5).bfloat16()
                   for S, h in ((Sq, H), (Sk, Hk), (Sk, Hk), (Sq, H))]
    seqlen = torch.tensor(seqlen, dtype=torch.int32)
    return (q, k, v, do, seqlen), _sha(q, k, v, do, seqlen)


def run_wrappers(cid, inputs, general=True):
    """(o, lse, dq, dk, dv) of a case through attention_fwd / attention_bwd; the dropout state is
    RngState(99) advanced once, site 5. general=False leaves Sk / Hk at None (self cases only)."""
    H, Hk, Sq, Sk, _, p, causal, fused = PARENT_CASES[cid]
    q, k, v, do, seqlen = [t.cuda() for t in inputs]
    rng = T.RngState(99, "cuda")
    rng.advance()
    o = torch.empty_like(q)
    lse = torch.empty(B * H, Sq, dtype=torch.float32, device="cuda")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    kw = dict(seqlen=seqlen, p_drop=p, rng=rng, site=5, causal=causal)
    if general:
        kw.update(Sk=Sk, Hk=Hk)
    T.attention_fwd(q, k, v, o, lse, B, H, Sq, **kw)
    T.set_fused_attention_bwd(fused)
    try:
        T.attention_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, Sq, **kw)
    finally:
        T.set_fused_attention_bwd(False)
    return o, lse, dq, dk, dv


def digests(outputs):
    return {name: _sha(t) for name, t in zip(OUTPUTS, outputs)}


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def assert_explicit_entry_is_self_attention(cid):
    """`ttdk_attn_fwd` / `ttdk_attn_bwd` called by hand with explicit Hk = H, Sq = Sk = S give, bit
    for bit, what the wrappers give with Sk / Hk left None, and what the parent commit's
    self-attention entry points gave (the recorded digests)."""
    H, Hk, S, Sk, _, p, causal, _ = PARENT_CASES[cid]
    assert Hk == H and Sk == S and p > 0
    inputs, _ = case_inputs(cid)
    want = run_wrappers(cid, inputs, general=False)
    q, k, v, do, seqlen = [t.cuda() for t in inputs]
    rng = T.RngState(99, "cuda")
    rng.advance()
    o, lse, dq, dk, dv = [torch.empty_like(t) for t in want]
    delta = torch.empty_like(lse)
    D, st = H * 64, T._lib.stream()
    T._lib.call("ttdk_attn_fwd", q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, o.data_ptr(), D,
                lse.data_ptr(), seqlen.data_ptr(), B, H, H, S, S, p, rng.t.data_ptr(), 5, int(causal), st)
    T._lib.call("ttdk_attn_bwd", q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, o.data_ptr(), D,
                do.data_ptr(), D, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), D, dk.data_ptr(), D,
                dv.data_ptr(), D, seqlen.data_ptr(), B, H, H, S, S, p, rng.t.data_ptr(), 5, int(causal), st)
    for name, a, b in zip(OUTPUTS, (o, lse, dq, dk, dv), want):
        assert torch.equal(a, b), name
    assert float(dq.float().abs().max()) > 0 and float(dk.float().abs().max()) > 0
    recorded = golden()["cases"][cid]
    assert digests((o, lse, dq, dk, dv)) == {n: recorded[n] for n in OUTPUTS}


if __name__ == "__main__":
    out = {"recorded_at_commit": sys.argv[2], "rocm": torch.version.hip, "cases": {}}
    for cid in PARENT_CASES:
        inputs, sha = case_inputs(cid)
        first, again = digests(run_wrappers(cid, inputs)), digests(run_wrappers(cid, inputs))
        assert first == again, (cid, "two runs, different bits")
        out["cases"][cid] = {"inputs": sha, **first}
        print(cid, first["o"][:12], first["dk"][:12], flush=True)
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
