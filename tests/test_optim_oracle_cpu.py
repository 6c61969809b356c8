"""The float64 optimizer reference of tests/optim_oracle.py, checked on the CPU: against
torch.optim where the two are defined alike, against a LAMB step worked out by hand, and at the
boundary steps of the schedules; then the project's CPU optimizers (train/flat.py) and the
reference itself in fp32 against it, on the cases and at the bars of tests/test_optimizers.py."""
import math

import pytest
import torch

import optim_oracle as O
from tensorflow_train_distributed_amd.train.flat import Schedule


def _two_vars():
    gen = torch.Generator().manual_seed(7)
    variables = [("a", (5, 3), True, True), ("b", (4,), True, True)]
    w0 = {n: torch.randn(shape, generator=gen, dtype=torch.float64) for n, shape, *_ in variables}
    # bounded away from 0: |g| in [0.5, 1.5]
    grads = [{n: (torch.rand(shape, generator=gen, dtype=torch.float64) + 0.5)
              * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
              for n, shape, *_ in variables} for _ in range(5)]
    return variables, w0, grads


def _torch_run(make, variables, w0, grads):
    ps = {n: w0[n].clone().requires_grad_(True) for n, *_ in variables}
    opt = make(list(ps.values()))
    for grad in grads:
        for n, p in ps.items():
            p.grad = grad[n].clone()
        opt.step()
    return {n: p.detach() for n, p in ps.items()}


@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
def test_sgd_matches_torch(momentum, nesterov):
    variables, w0, grads = _two_vars()
    hp = {"opt": "sgd", "momentum": momentum, "nesterov": nesterov, "weight_decay": 0.1,
          "schedule": {"kind": 0, "base_lr": 0.05}}
    got = O.run(variables, w0, grads, hp)["w"]
    ref = _torch_run(lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=momentum, nesterov=nesterov,
                                                weight_decay=0.1), variables, w0, grads)
    for n in ref:
        torch.testing.assert_close(got[n], ref[n], rtol=1e-12, atol=0)


@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_matches_torch(decoupled):
    """torch: m_hat / (sqrt(v_hat) + eps); TF: lr_t * m / (sqrt(v) + eps). With eps = 1e-30 and
    gradients bounded away from 0 the two placements of eps coincide."""
    variables, w0, grads = _two_vars()
    hp = {"opt": "adam", "decoupled": decoupled, "weight_decay": 0.1, "eps": 1e-30,
          "schedule": {"kind": 0, "base_lr": 1e-2}}
    got = O.run(variables, w0, grads, hp)["w"]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    ref = _torch_run(lambda ps: cls(ps, lr=1e-2, betas=(0.9, 0.999), eps=1e-30, weight_decay=0.1),
                     variables, w0, grads)
    for n in ref:
        torch.testing.assert_close(got[n], ref[n], rtol=1e-10, atol=0)


def test_lamb_step_by_hand():
    """One LAMB step, b1 = 0.5, b2 = 0.75, eps = 0, wd = 0.5, lr = 0.1 (all exact in binary).
    At t = 1: m_hat = g and v_hat = g*g, so m_hat / sqrt(v_hat) = sign(g).

    p = [3, -4], g = [2, -8], decays:     u = [1, -1] + 0.5*[3, -4] = [2.5, -3]
        |w| = 5, |u| = sqrt(15.25), trust = 5/sqrt(15.25); w = [3, -4] - 0.1*trust*[2.5, -3]
    z = [0, 0, 0], g = [1, -2, 4], no decay: u = [1, -1, 1], |w| = 0 -> trust = 1
        w = -0.1*[1, -1, 1]
    state: m = 0.5*g, v = 0.25*g*g."""
    variables = [("p", (2,), True, True), ("z", (3,), False, True)]
    w0 = {"p": torch.tensor([3.0, -4.0], dtype=torch.float64), "z": torch.zeros(3, dtype=torch.float64)}
    grads = [{"p": torch.tensor([2.0, -8.0], dtype=torch.float64),
              "z": torch.tensor([1.0, -2.0, 4.0], dtype=torch.float64)}]
    hp = {"opt": "lamb", "beta1": 0.5, "beta2": 0.75, "eps": 0.0, "weight_decay": 0.5,
          "schedule": {"kind": 0, "base_lr": 0.1}}
    out = O.run(variables, w0, grads, hp)
    trust = 5.0 / math.sqrt(15.25)  # 1.2803687993289596
    exp_p = torch.tensor([3.0 - 0.25 * trust, -4.0 + 0.3 * trust], dtype=torch.float64)
    torch.testing.assert_close(out["w"]["p"], exp_p, rtol=1e-14, atol=0)
    torch.testing.assert_close(out["w"]["p"], torch.tensor([2.6799078001677601, -3.6158893602013121],
                                                           dtype=torch.float64), rtol=1e-14, atol=0)
    torch.testing.assert_close(out["w"]["z"], torch.tensor([-0.1, 0.1, -0.1], dtype=torch.float64),
                               rtol=1e-15, atol=0)
    assert torch.equal(out["m"]["p"], torch.tensor([1.0, -4.0], dtype=torch.float64))
    assert torch.equal(out["v"]["p"], torch.tensor([1.0, 16.0], dtype=torch.float64))
    assert torch.equal(out["m"]["z"], torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64))
    assert torch.equal(out["v"]["z"], torch.tensor([0.25, 1.0, 4.0], dtype=torch.float64))
    assert out["norms"][0]["p"] == (25.0, 15.25) and out["norms"][0]["z"] == (0.0, 3.0)


def test_schedule_matches_oracle_at_boundaries():
    for sched, steps in O.SCHEDULE_BOUNDARIES:
        mine = Schedule(kind=sched["kind"], base_lr=sched["base_lr"], decay_steps=sched.get("decay_steps", 1.0),
                        decay_rate=sched.get("decay_rate", 1.0), staircase=sched.get("staircase", False),
                        warmup_steps=sched.get("warmup_steps", 0.0), end_lr=sched.get("end_lr", 0.0),
                        power=sched.get("power", 1.0), total_steps=sched.get("total_steps", 1.0))
        for s in steps:
            assert mine.value(s) == pytest.approx(O.schedule_lr(sched, s), rel=1e-14, abs=0), (sched, s)


def test_schedule_oracle_reference_values():
    """The reference example's staircase (0.1 * 0.96^floor(step/468)) and the shape of the
    warm-up schedules, by value."""
    exp = O.SCHEDULE_BOUNDARIES[0][0]
    assert [O.schedule_lr(exp, s) for s in (0, 467, 468, 469, 935, 936)] == pytest.approx(
        [0.1, 0.1, 0.096, 0.096, 0.096, 0.09216], rel=1e-14)
    for kind in (2, 3):
        s = {"kind": kind, "base_lr": 0.01, "warmup_steps": 100.0, "total_steps": 1000.0, "end_lr": 1e-4,
             "power": 2.0}
        assert O.schedule_lr(s, 0) == pytest.approx(1e-4, rel=1e-14)     # base * 1/warmup
        assert O.schedule_lr(s, 99) == pytest.approx(1e-2, rel=1e-14)    # base * warmup/warmup
        assert O.schedule_lr(s, 1000) == pytest.approx(1e-4, rel=1e-12)  # end_lr
        assert O.schedule_lr(s, 1005) == pytest.approx(1e-4, rel=1e-12)
    poly = {"kind": 2, "base_lr": 0.01, "warmup_steps": 100.0, "total_steps": 1000.0, "end_lr": 1e-4, "power": 2.0}
    assert O.schedule_lr(poly, 100) == pytest.approx((0.01 - 1e-4) * 0.81 + 1e-4, rel=1e-14)
    cosine = dict(poly, kind=3)
    assert O.schedule_lr(cosine, 100) == pytest.approx(0.01, rel=1e-14)
    assert O.schedule_lr(cosine, 550) == pytest.approx(1e-4 + 0.5 * (0.01 - 1e-4), rel=1e-12)  # half way


@pytest.mark.parametrize("case", list(O.CASES))
def test_cpu_flat_optimizers_match_oracle(case):
    params, opt = O.make_flat(case, "cpu", compute_dtype=None)
    w0, _ = O.inputs(bool(O.CASES[case].get("big")))
    ref = O.reference(case)
    for i, flat in enumerate(O.flat_grads(case, params)):
        params.grad.copy_(flat)
        opt.step()
        assert float(opt.hyper[0]) == pytest.approx(ref["lr"][i], rel=2e-6), i
    assert int(opt.step_t) == O.STEPS
    state = {k: O.by_name(params, buf) for k, buf in O.state_buffers(opt).items()}
    figs = O.check_against(ref, w0, params.var, state, label=case)
    print(case, "worst", O.worst(figs))
    assert torch.equal(params.var["frozen"], w0["frozen"])


@pytest.mark.parametrize("case", list(O.CASES))
def test_fp32_oracle_within_half_of_each_bar(case):
    """The bars of the GPU tests are reachable in fp32 on these inputs: the reference itself, run
    in float32, stays within half of each."""
    w0, grads = O.inputs(bool(O.CASES[case].get("big")))
    ref = O.reference(case)
    got = O.run(O.variables(case), w0, grads, O.oracle_hp(case), dtype=torch.float32)
    state = {k: got[k] for k in ("m", "v", "mom") if k in got}
    figs = O.check_against(ref, w0, got["w"], state, w_bar=O.W_BAR / 2, state_bar=O.STATE_BAR / 2, label=case)
    print(case, "worst", O.worst(figs))
