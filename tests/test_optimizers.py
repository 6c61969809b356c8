"""The fused flat optimizers (csrc/kernels/optim.hip through train/flat.py) and the device
learning-rate schedule against the float64 reference of tests/optim_oracle.py, which is written
from the definitions of SGD, Adam and LAMB and shares no code with either.

Per variable: the weights within 2e-3 of the distance the variable moved (a wrong term of the
update cannot hide under |w|), the state within 1e-5 of its largest entry, the bf16 compute copy
the exact rounding of the master, and nothing written outside the chunk table (sentinels in the
alignment padding and in the non-trainable variable). tests/test_optim_oracle_cpu.py shows that
the reference run in fp32 stays within half of these bars on the same inputs.

Two bars are this file's own. The clip's sum of squares within 1e-5 of the reference: each thread
adds at most 64 squares in turn and the rest is folded pairwise, so rounding stays below about
(64 + 30) * 2^-24 = 6e-6, while the padding and the non-trainable slots, which must not count,
would add 1e-4 (6e-3 without `big`). LAMB's per-variable sums of w^2 and u^2 within 1e-4: the
same rounding plus that of u from fp32 m and v, while one chunk of 258 dropped changes them by
4e-3."""
import pytest
import torch

import optim_oracle as O
from tensorflow_train_distributed_amd.train import flat as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CLIPPED = [c for c, hp in O.CASES.items() if hp.get("max_grad_norm", 0.0) > 0]


def _sentinels(params, opt):
    """Fill every slot outside the chunk table, in every buffer a step may write, with noise;
    returns the mask and {buffer name: (tensor, expected contents of those slots)}."""
    mask = O.outside_mask(params).to(DEV)
    bufs = dict(O.state_buffers(opt), master=params.master, compute=params.compute)
    if hasattr(opt, "u"):
        bufs["u"] = opt.u
    gen = torch.Generator().manual_seed(5)
    noise = (torch.randn(params.numel, generator=gen) * 100).to(DEV)
    expected = {}
    for k, b in bufs.items():
        b[mask] = noise[mask].to(b.dtype)
        expected[k] = (b, b[mask].clone())
    return mask, expected


def _run(case, first=0, last=O.STEPS, state_from=None, check_lr=False):
    """A fresh optimizer of `case`, stepped over gradients first..last-1."""
    params, opt = O.make_flat(case, DEV)
    if state_from is not None:
        p0, o0 = state_from
        params.master.copy_(p0.master)
        opt.m.copy_(o0.m)
        opt.v.copy_(o0.v)
        opt.set_step(first)
    ref = O.reference(case)
    grads = O.flat_grads(case, params)
    for i in range(first, last):
        params.grad.copy_(grads[i])
        opt.step()
        if check_lr:
            torch.testing.assert_close(float(opt.hyper[F.H_LR]), ref["lr"][i], rtol=2e-6, atol=0)
            assert int(opt.step_t) == i + 1
    return params, opt


_eager = {}


def _eager_master(case):
    """Master weights and LAMB norms after the 6 eager steps of `case` (computed once)."""
    if case not in _eager:
        params, opt = _run(case)
        _eager[case] = (params.master.clone(), opt.seg_norms.clone() if hasattr(opt, "seg_norms") else None)
    return _eager[case]


@pytest.mark.parametrize("case", list(O.CASES))
def test_matches_oracle(case):
    hp = O.CASES[case]
    params, opt = O.make_flat(case, DEV)
    w0, _ = O.inputs(bool(hp.get("big")))
    ref = O.reference(case)
    mask, sentinels = _sentinels(params, opt)
    for i, flat in enumerate(O.flat_grads(case, params)):
        params.grad.copy_(flat)  # padding and the frozen variable carry N(0,1) gradients
        opt.step()
        torch.testing.assert_close(float(opt.hyper[F.H_LR]), ref["lr"][i], rtol=2e-6, atol=0)
        assert int(opt.step_t) == i + 1
    state = {k: O.by_name(params, buf) for k, buf in O.state_buffers(opt).items()}
    figs = O.errors(ref, w0, params.var, state)
    print(case, "worst", O.worst(figs))
    if case in CLIPPED:
        want = ref["sumsq"][-1] * hp.get("grad_mult", 1.0) ** 2
        print(case, "sumsq", float(opt._sumsq), want)
        torch.testing.assert_close(float(opt._sumsq), want, rtol=1e-5, atol=0)
    O.check_against(ref, w0, params.var, state, label=case)
    if hp["opt"] == "lamb":
        for seg, s in enumerate(params.specs):
            if s.trainable:
                got = opt.seg_norms[2 * seg:2 * seg + 2].double().cpu()
                torch.testing.assert_close(got, torch.tensor(ref["norms"][-1][s.name], dtype=torch.float64),
                                           rtol=1e-4, atol=0, msg=lambda m, n=s.name: "%s %s: %s" % (case, n, m))
    for s in params.specs:
        if s.trainable:  # the 4-wide path and the scalar tail both round to nearest even
            assert torch.equal(params.c[s.name], params.var[s.name].bfloat16()), (case, s.name)
    for k, (buf, want) in sentinels.items():
        assert torch.equal(buf[mask], want), (case, k, "written outside the chunk table")


def test_lamb_is_deterministic():
    """Two fresh optimizers on the same inputs end bit-identical (no float atomics in the norms:
    data-parallel replicas never drift apart)."""
    master, norms = _eager_master("lamb_bert")
    params, opt = _run("lamb_bert")
    assert torch.equal(params.master, master)
    assert torch.equal(opt.seg_norms, norms)


@pytest.mark.parametrize("case", ["adam_l2_clip", "lamb_bert"])
def test_resume_is_bit_identical(case):
    """3 steps, the weights and the state copied into a fresh optimizer, set_step(3), 3 more
    steps: the same bits as 6 steps in one go."""
    master, _ = _eager_master(case)
    half = _run(case, 0, 3)
    params, opt = _run(case, 3, O.STEPS, state_from=half, check_lr=True)
    assert torch.equal(params.master, master)


def test_graph_replay_follows_schedule():
    """One captured FlatLAMB.step() (schedule kernel, clip norm, the three LAMB kernels; a single
    stream), replayed 6 times with a new gradient each: bit-identical to 6 eager steps, the
    learning rate following the warm-up from the device step counter without re-capture."""
    from tensorflow_train_distributed_amd.utils.graphs import capture
    case = "lamb_bert"
    master, _ = _eager_master(case)
    params, opt = O.make_flat(case, DEV)
    ref = O.reference(case)
    grads = O.flat_grads(case, params)
    start = params.master.clone()
    params.grad.copy_(grads[0])
    step, _ = capture(opt.step, warmup=1)  # the warm-up call is a real step: undo it
    params.master.copy_(start)
    opt.m.zero_()
    opt.v.zero_()
    opt.set_step(0)
    for i in range(O.STEPS):
        params.grad.copy_(grads[i])
        step.replay()
        torch.testing.assert_close(float(opt.hyper[F.H_LR]), ref["lr"][i], rtol=2e-6, atol=0)
        assert int(opt.step_t) == i + 1
    assert torch.equal(params.master, master)
    for s in params.specs:
        if s.trainable:
            assert torch.equal(params.c[s.name], params.var[s.name].bfloat16()), s.name


def _tiny_opt(sched=None, **kw):
    params = F.FlatParams([F.ParamSpec("w", (8,))], DEV)
    return F.FlatAdam(params, sched or F.Schedule(), **kw)


def test_device_schedule_at_boundaries():
    """H_LR of lr_schedule_kernel against the float64 schedule: rtol 2e-6 = 16 fp32 ulp for one
    powf or cosf, a divide and two multiplies. increment=False leaves the step alone."""
    for sched, steps in O.SCHEDULE_BOUNDARIES:
        opt = _tiny_opt(F.Schedule(kind=sched["kind"], base_lr=sched["base_lr"],
                                   decay_steps=sched.get("decay_steps", 1.0), decay_rate=sched.get("decay_rate", 1.0),
                                   staircase=sched.get("staircase", False), warmup_steps=sched.get("warmup_steps", 0.0),
                                   end_lr=sched.get("end_lr", 0.0), power=sched.get("power", 1.0),
                                   total_steps=sched.get("total_steps", 1.0)))
        for s in steps:
            opt.set_step(s)
            opt._prologue(increment=False)
            assert int(opt.step_t) == s
            torch.testing.assert_close(float(opt.hyper[F.H_LR]), O.schedule_lr(sched, s), rtol=2e-6, atol=0,
                                       msg=lambda m, s=s: "%s step %d: %s" % (sched, s, m))
            opt._prologue()
            assert int(opt.step_t) == s + 1
            # evaluated at the step BEFORE the increment
            torch.testing.assert_close(float(opt.hyper[F.H_LR]), O.schedule_lr(sched, s), rtol=2e-6, atol=0)


def test_device_bias_corrections():
    """H_BC1 / H_BC2 = 1 - beta^t at t = step + 1, rtol 2 * 2^-24 / (1 - beta): the cancellation
    bound of 1 - powf(beta, t) with beta rounded to fp32 (1.2e-4 for beta2 = 0.999)."""
    b1, b2 = 0.9, 0.999
    opt = _tiny_opt(beta1=b1, beta2=b2)
    for t in (1, 2, 3, 10, 100, 1000, 2000):
        opt.set_step(t - 1)
        opt._prologue(increment=False)
        bc1, bc2 = O.bias_corrections(b1, b2, t - 1)
        h = opt.hyper.double().cpu()
        torch.testing.assert_close(float(h[F.H_BC1]), bc1, rtol=2 * 2.0 ** -24 / (1 - b1), atol=0)
        torch.testing.assert_close(float(h[F.H_BC2]), bc2, rtol=2 * 2.0 ** -24 / (1 - b2), atol=0)
