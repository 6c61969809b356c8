"""What the optimizer test files share (a plain module, imported by them):

* a float64 reference of the optimizers and learning-rate schedules, written from their
  definitions and not from train/flat.py or optim.hip: torch on the CPU, one tensor per variable,
  no flat buffer, no padding, no chunk table (`schedule_lr`, `bias_corrections`, `run`);
* the variables, inputs, case table and bars of tests/test_optimizers.py (GPU) and
  tests/test_optim_oracle_cpu.py (`VARS`, `BIG`, `CASES`, `inputs`, `reference`, `make_flat`,
  `flat_grads`, `check_against`).

Definitions (w: weights, g: gradient, t = step + 1, `step` the global step BEFORE the update):

  gradient     g <- grad_scale * g; if max_grad_norm > 0 and the global norm n of all TRAINABLE
               g exceeds it, g <- g * max_grad_norm / n
  SGD          g += wd*w; acc = mu*acc + g; w -= lr*acc      (Nesterov: w -= lr*(g + mu*acc))
  Adam (TF)    [L2: g += wd*w]  m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g
               w -= lr*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps)   [decoupled: w -= lr*wd*w_old]
  LAMB         m, v as Adam (no L2); u = (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps) + wd*w;
               trust = |w|/|u| per variable, 1 if either norm is 0; w -= lr*trust*u
  schedules    0 constant; 1 base*rate^(step/decay_steps), the exponent floored with staircase;
               2 base*(step+1)/warmup while step < warmup, then
                 (base-end)*(1 - min(step,total)/total)^power + end;
               3 the same warm-up, then end + (base-end)/2 * (1 + cos(pi*min(1, (step-warmup) /
                 max(1, total-warmup))))
  wd is `weight_decay` on variables that decay and 0 on the others; variables with
  trainable=False are never read or written.
"""
import math

import torch

# ------------------------------------------------------------------ the reference


def schedule_lr(sched, step):
    """Learning rate at global step `step` (a python float, double precision)."""
    kind = sched.get("kind", 0)
    base = sched["base_lr"]
    end = sched.get("end_lr", 0.0)
    warm = sched.get("warmup_steps", 0.0)
    total = sched.get("total_steps", 1.0)
    if kind == 0:
        return base
    if kind == 1:
        e = step / sched["decay_steps"]
        if sched.get("staircase", False):
            e = math.floor(e)
        return base * sched["decay_rate"] ** e
    if kind in (2, 3) and warm > 0 and step < warm:
        return base * (step + 1) / warm
    if kind == 2:
        return (base - end) * (1.0 - min(step, total) / total) ** sched.get("power", 1.0) + end
    if kind == 3:
        frac = min(1.0, (step - warm) / max(1.0, total - warm))
        return end + 0.5 * (base - end) * (1.0 + math.cos(math.pi * frac))
    raise ValueError(kind)


def bias_corrections(beta1, beta2, step):
    t = step + 1
    return 1.0 - beta1 ** t, 1.0 - beta2 ** t


def run(variables, w0, grads, hp, dtype=torch.float64):
    """Step the optimizer `hp` over `grads` (one {name: tensor} per step) from weights `w0`.

    variables: [(name, shape, weight_decay?, trainable?)]. Returns a dict with the final `w`,
    the state `m` / `v` (Adam, LAMB) or `mom` (momentum SGD) per variable, and per step `lr`,
    `sumsq` (sum of squares of the unscaled trainable gradients) and `norms` ({name: (sum w^2,
    sum u^2)} of LAMB, taken before the weights move). dtype=float32 runs the same arithmetic
    in single precision (the schedule and the clip factor stay python floats)."""
    opt = hp["opt"]
    wd0 = hp.get("weight_decay", 0.0)
    mu = hp.get("momentum", 0.0)
    b1, b2 = hp.get("beta1", 0.9), hp.get("beta2", 0.999)
    eps = hp.get("eps", 1e-6 if opt == "lamb" else 1e-8)
    gscale = hp.get("grad_scale", 1.0)
    max_norm = hp.get("max_grad_norm", 0.0)
    step = hp.get("start_step", 0)
    live = [(n, wd0 if decay else 0.0) for n, _, decay, trainable in variables if trainable]
    w = {n: w0[n].to(dtype).clone() for n, *_ in variables}
    zeros = lambda: {n: torch.zeros_like(w[n]) for n, _ in live}  # noqa: E731
    m, v, mom = zeros(), zeros(), zeros()
    out = {"lr": [], "sumsq": [], "norms": []}
    for grad in grads:
        lr = schedule_lr(hp["schedule"], step)
        bc1, bc2 = bias_corrections(b1, b2, step)
        ss = sum(float((grad[n].double() ** 2).sum()) for n, _ in live)
        scale = gscale
        if max_norm > 0 and math.sqrt(ss) * gscale > max_norm:
            scale = max_norm / math.sqrt(ss)
        norms = {}
        for n, wd in live:
            g = grad[n].to(dtype) * scale
            if opt == "sgd":
                g = g + wd * w[n]
                if mu > 0:
                    mom[n] = mu * mom[n] + g
                    w[n] = w[n] - lr * (g + mu * mom[n] if hp.get("nesterov") else mom[n])
                else:
                    w[n] = w[n] - lr * g
                continue
            if opt == "adam" and not hp.get("decoupled"):
                g = g + wd * w[n]
            m[n] = b1 * m[n] + (1 - b1) * g
            v[n] = b2 * v[n] + (1 - b2) * g * g
            if opt == "adam":
                new = w[n] - lr * math.sqrt(bc2) / bc1 * m[n] / (v[n].sqrt() + eps)
                if hp.get("decoupled"):
                    new = new - lr * wd * w[n]
                w[n] = new
            elif opt == "lamb":
                u = (m[n] / bc1) / ((v[n] / bc2).sqrt() + eps) + wd * w[n]
                sw, su = float((w[n].double() ** 2).sum()), float((u.double() ** 2).sum())
                norms[n] = (sw, su)
                trust = math.sqrt(sw) / math.sqrt(su) if sw > 0 and su > 0 else 1.0
                w[n] = w[n] - lr * trust * u
            else:
                raise ValueError(opt)
        out["lr"].append(lr)
        out["sumsq"].append(ss)
        out["norms"].append(norms)
        step += 1
    out["w"] = w
    out["trainable"] = [n for n, _ in live]
    if opt == "sgd":
        if mu > 0:
            out["mom"] = mom
    else:
        out["m"], out["v"] = m, v
    return out


# ------------------------------------------------------------------ shared cases
# (name, shape, weight_decay?, trainable?). 16384 is the chunk length of the flat optimizers.
VARS = [
    ("k0", (300, 70), True, True),      # 21000: crosses a chunk boundary
    ("b0", (70,), False, True),         # zero-initialised (trust = 1), no decay, len % 4 == 2
    ("s0", (), True, True),             # a scalar
    ("t1", (16385,), True, True),       # a chunk of length 1; len % 4 == 1
    ("t3", (16387,), True, True),       # len % 4 == 3
    ("full", (16384,), True, True),     # exactly one chunk
    ("frozen", (96,), True, False),     # never touched
]
# 258 chunks: the smallest variable whose chunks exceed lamb_segnorm_kernel's 256 threads
BIG = ("big", (257 * 16384 + 5,), True, True)

STEPS = 6
WD = 0.1

W_BAR = 2e-3      # max|w - w_ref| / max|w_ref(T) - w(0)|, per variable
STATE_BAR = 1e-5  # max|s - s_ref| / max|s_ref|, per variable (m, v, momentum buffer)

_EXP = {"kind": 1, "base_lr": 0.1, "decay_steps": 2.0, "decay_rate": 0.5, "staircase": True}
_BERT = {"kind": 2, "base_lr": 1e-2, "warmup_steps": 3.0, "total_steps": 10.0}

# name -> hyper-parameters. "grad_mult": the gradients fed are that multiple of the common ones
# (undone by grad_scale). N(0,1) gradients over these variables have a global norm of about 265
# (2070 with `big`), so max_grad_norm 1.0 and 100.0 clip and 1e4 does not.
CASES = {
    "sgd": {"opt": "sgd", "schedule": {"kind": 0, "base_lr": 0.05}},
    "momentum_staircase": {"opt": "sgd", "momentum": 0.9, "schedule": _EXP},
    "nesterov": {"opt": "sgd", "momentum": 0.9, "nesterov": True, "schedule": _EXP},
    "adam_l2_clip": {"opt": "adam", "schedule": {"kind": 0, "base_lr": 1e-3}, "max_grad_norm": 1.0},
    "adamw": {"opt": "adam", "decoupled": True, "schedule": {"kind": 0, "base_lr": 1e-3}},
    "lamb_bert": {"opt": "lamb", "schedule": _BERT, "max_grad_norm": 1.0, "big": True},
    "lamb_cosine": {"opt": "lamb", "big": True,
                    "schedule": {"kind": 3, "base_lr": 1e-2, "warmup_steps": 2.0, "total_steps": 10.0,
                                 "end_lr": 1e-3}},
    "lamb_poly2": {"opt": "lamb", "big": True,
                   "schedule": {"kind": 2, "base_lr": 1e-2, "warmup_steps": 2.0, "total_steps": 10.0,
                                "power": 2.0, "end_lr": 1e-4}},
    "momentum_clip_gradscale": {"opt": "sgd", "momentum": 0.9, "schedule": {"kind": 0, "base_lr": 0.05},
                                "max_grad_norm": 100.0, "grad_scale": 1.0 / 128, "grad_mult": 128.0},
    "momentum_below_clip": {"opt": "sgd", "momentum": 0.9, "schedule": {"kind": 0, "base_lr": 0.05},
                            "max_grad_norm": 1e4},
}
for _hp in CASES.values():
    _hp["weight_decay"] = WD

# (schedule, steps): the reference example's staircase (0.1 * 0.96^floor(step/468)) around its
# first two decays; warm-up then polynomial (power 1 and 2) or cosine decay, end_lr > 0, at
# warmup-1, warmup, total and total+5.
_WARM = {"base_lr": 4e-3, "warmup_steps": 100.0, "total_steps": 1000.0, "end_lr": 1e-4}
SCHEDULE_BOUNDARIES = [
    ({"kind": 1, "base_lr": 0.1, "decay_steps": 468.0, "decay_rate": 0.96, "staircase": True},
     (0, 467, 468, 469, 935, 936)),
    (dict(_WARM, kind=2, power=1.0), (99, 100, 1000, 1005)),
    (dict(_WARM, kind=2, power=2.0), (99, 100, 1000, 1005)),
    (dict(_WARM, kind=3), (99, 100, 1000, 1005)),
]

_inputs = {}


def variables(case):
    return VARS + [BIG] if CASES[case].get("big") else VARS


def numel(shape):
    return int(math.prod(shape))


def inputs(big):
    """(w0, grads): fp32 N(0,1) weights (b0 zero) and STEPS gradients per variable, seeded;
    computed once and shared (do not modify)."""
    if big not in _inputs:
        gen = torch.Generator().manual_seed(1234 + int(big))
        vs = VARS + [BIG] if big else VARS
        w0 = {n: torch.randn(shape, generator=gen) for n, shape, *_ in vs}
        w0["b0"] = torch.zeros(70)
        grads = [{n: torch.randn(shape, generator=gen) for n, shape, *_ in vs} for _ in range(STEPS)]
        _inputs[big] = (w0, grads)
    return _inputs[big]


_refs = {}


def reference(case):
    """The float64 result of `case` on the shared inputs (computed once)."""
    if case not in _refs:
        w0, grads = inputs(bool(CASES[case].get("big")))
        _refs[case] = run(variables(case), w0, grads, oracle_hp(case))
    return _refs[case]


def oracle_hp(case):
    """Hyper-parameters of the oracle: it is fed the common gradients, so a case that multiplies
    the gradients and divides by grad_scale is, for it, the case without either."""
    hp = dict(CASES[case])
    mult = hp.pop("grad_mult", 1.0)
    assert hp.get("grad_scale", 1.0) * mult == 1.0
    hp.pop("grad_scale", None)
    return hp


# ------------------------------------------------------------------ the project's optimizers
def make_flat(case, device, compute_dtype=torch.bfloat16):
    """(FlatParams, optimizer) of `case` holding the shared initial weights."""
    from tensorflow_train_distributed_amd.train import flat as F
    hp = CASES[case]
    specs = [F.ParamSpec(n, shape, None, weight_decay=decay, trainable=trainable)
             for n, shape, decay, trainable in variables(case)]
    params = F.FlatParams(specs, device, compute_dtype=compute_dtype)
    w0, _ = inputs(bool(hp.get("big")))
    with torch.no_grad():
        for n in params.names():
            params.var[n].copy_(w0[n])
    params.refresh_compute()
    s = hp["schedule"]
    sched = F.Schedule(kind=s["kind"], base_lr=s["base_lr"], decay_steps=s.get("decay_steps", 1.0),
                       decay_rate=s.get("decay_rate", 1.0), staircase=s.get("staircase", False),
                       warmup_steps=s.get("warmup_steps", 0.0), end_lr=s.get("end_lr", 0.0),
                       power=s.get("power", 1.0), total_steps=s.get("total_steps", 1.0))
    kw = {"weight_decay": hp["weight_decay"], "max_grad_norm": hp.get("max_grad_norm", 0.0)}
    if hp["opt"] == "sgd":
        opt = F.FlatSGD(params, sched, momentum=hp.get("momentum", 0.0), nesterov=hp.get("nesterov", False), **kw)
    elif hp["opt"] == "adam":
        opt = F.FlatAdam(params, sched, decoupled=hp.get("decoupled", False), **kw)
    else:
        opt = F.FlatLAMB(params, sched, **kw)
    if "grad_scale" in hp:
        opt.hyper[F.H_GRADSCALE] = hp["grad_scale"]
    return params, opt


def outside_mask(params):
    """True on the slots of the flat buffer no optimizer may write: alignment padding and the
    variables with trainable=False."""
    mask = torch.ones(params.numel, dtype=torch.bool)
    for s in params.specs:
        if s.trainable:
            o = params.offsets[s.name]
            mask[o:o + numel(s.shape)] = False
    return mask


def flat_grads(case, params):
    """The case's gradients as flat fp32 buffers (CPU), one per step: the variables' slots hold
    the shared gradients times grad_mult, every other slot (padding, frozen) N(0,1) noise."""
    hp = CASES[case]
    _, grads = inputs(bool(hp.get("big")))
    gen = torch.Generator().manual_seed(99)
    out = []
    for grad in grads:
        flat = torch.randn(params.numel, generator=gen)
        for s in params.specs:
            if s.trainable:
                o = params.offsets[s.name]
                flat[o:o + numel(s.shape)] = grad[s.name].reshape(-1) * hp.get("grad_mult", 1.0)
        out.append(flat)
    return out


def state_buffers(opt):
    """{name: flat state tensor} of a Flat* optimizer."""
    return {k: getattr(opt, k) for k in ("m", "v", "mom") if getattr(opt, k, None) is not None}


def errors(ref, w0, got_w, got_state):
    """Per variable, the figures the bars apply to: {name: {"w": err / distance moved,
    "m" | "v" | "mom": err / max|ref|}} of results `got_*` ({name: tensor}) against `ref`."""
    out = {}
    for n in ref["trainable"]:
        wr = ref["w"][n]
        moved = float((wr - w0[n].double()).abs().max())
        fig = {"w": float((got_w[n].double().cpu() - wr).abs().max()) / moved}
        for k, got in got_state.items():
            r = ref[k][n]
            fig[k] = float((got[n].double().cpu() - r).abs().max()) / float(r.abs().max())
        out[n] = fig
    return out


def worst(figs):
    """{quantity: (largest figure, variable)} of an `errors` result."""
    out = {}
    for n, f in figs.items():
        for k, v in f.items():
            if k not in out or not v <= out[k][0]:
                out[k] = (v, n)
    return out


def check_against(ref, w0, got_w, got_state, w_bar=W_BAR, state_bar=STATE_BAR, label=""):
    figs = errors(ref, w0, got_w, got_state)
    bad = {n: f for n, f in figs.items()
           if not all(v <= (w_bar if k == "w" else state_bar) for k, v in f.items())}
    assert not bad, (label, bad)
    return figs


def by_name(params, flat):
    """{name: view of `flat`} for the variables of `params`."""
    return {s.name: flat[params.offsets[s.name]:params.offsets[s.name] + numel(s.shape)].view(tuple(s.shape))
            for s in params.specs}
