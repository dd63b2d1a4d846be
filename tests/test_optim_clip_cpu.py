"""Host half of global-norm clipping and AdamW: the fourth C-ABI header (include/t4r_hip_optim.h), its size query and argument
checks, the warm-up schedules against transformers.optimization, and what optim.FusedAdam does without a device.  Nothing here
needs a GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

from transformers4rec_amd import _lib, ops, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- header and ABI
def test_fourth_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_optim.h")
    assert len(syms) == 4
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_optim.h but not exported"
    text = open(_lib.header_path("t4r_hip_optim.h")).read()
    for name in ("t4r_grad_sumsq", "t4r_grad_clip_coef", "t4r_adamw_step"):
        decl = text[: text.index("int " + name + "(void* stream")]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment and "trainer.py" in comment, name
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"


def documented_parts(n):
    """include/t4r_hip_optim.h: min(max(ceil(floor(n / 4) / 256), 1), 2048); 0 for n <= 0"""
    return 0 if n <= 0 else min(max(-(-(n // 4) // 256), 1), 2048)


def test_sumsq_parts_is_the_documented_pure_function():
    lib = _lib.load()
    assert "min(max(ceil(floor(n / 4) / 256), 1), 2048)" in open(_lib.header_path("t4r_hip_optim.h")).read()
    ns = [-5, 0, 1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 70_001, 850_000, 2048 * 1024 - 1, 2048 * 1024, 2048 * 1024 + 4,
          12_800_128, 1 << 31, (1 << 33) + 7]
    got = [lib.t4r_grad_sumsq_parts(n) for n in ns]
    assert got == [documented_parts(n) for n in ns]
    assert got[:3] == [0, 0, 1] and max(got) == 2048 and got == sorted(got)
    assert [lib.t4r_grad_sumsq_parts(n) for n in range(1, 6000, 37)] == [documented_parts(n) for n in range(1, 6000, 37)]
    assert ops.grad_sumsq_parts(12_800_128) == 2048


def test_argument_errors_come_back_as_messages():
    lib = _lib.load()
    err = lib.t4r_last_error
    one, odd4, odd2 = ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(66)       # non-null, never dereferenced
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    # t4r_grad_sumsq
    assert lib.t4r_grad_sumsq(None, None, 0, None) == 0 and lib.t4r_grad_sumsq(None, None, -3, None) == 0     # nothing to do
    assert lib.t4r_grad_sumsq(None, None, 8, None) < 0 and b"grad_sumsq: grad and part must not be null" in err()
    assert lib.t4r_grad_sumsq(None, one, 8, None) < 0 and b"must not be null" in err()
    assert lib.t4r_grad_sumsq(None, odd4, 8, one) < 0 and b"grad_sumsq: grad must be 16-byte aligned" in err()
    assert lib.t4r_grad_sumsq(None, one, 8, odd4) < 0 and b"grad_sumsq: part must be 8-byte aligned" in err()
    # t4r_grad_clip_coef
    for bad in (0.0, -1.0, float("nan")):
        assert lib.t4r_grad_clip_coef(None, one, 4, 1.0, bad, one) < 0 and b"max_norm must be greater than 0" in err()
    assert lib.t4r_grad_clip_coef(None, one, 0, 1.0, 1.0, one) < 0 and b"n_part must be at least 1" in err()
    assert lib.t4r_grad_clip_coef(None, None, 4, 1.0, 1.0, None) < 0 and b"grad_clip_coef: part and out2 must not be null" in err()
    assert lib.t4r_grad_clip_coef(None, odd4, 4, 1.0, 1.0, one) < 0 and b"8-byte" in err()
    assert lib.t4r_grad_clip_coef(None, one, 4, 1.0, 1.0, odd2) < 0 and b"4-byte aligned" in err()

    # t4r_adamw_step
    def adamw(p=one, g=one, m=one, v=one, n=100, step=1, coef=None, lo=0, hi=0, part=None):
        return lib.t4r_adamw_step(None, p, g, m, v, n, step, *hp, 1, 1.0, 1, coef, lo, hi, part)

    assert adamw(None, None, None, None, n=0) == 0                                         # nothing to do
    assert adamw(step=0) < 0 and b"adamw: step is 1-based" in err()
    assert adamw(None, None, None, None, step=-2) < 0 and b"step is 1-based" in err()
    assert adamw(None, None, None, None) < 0 and b"adamw: buffers must not be null" in err()
    for k in range(4):
        bufs = [odd4 if i == k else one for i in range(4)]
        assert adamw(*bufs) < 0 and b"adamw: buffers must be 16-byte aligned" in err()
    assert adamw(coef=odd2) < 0 and b"clip_coef must be 4-byte aligned" in err()
    for lo, hi in ((5, 5), (6, 5), (-1, 10), (0, 101)):
        assert adamw(lo=lo, hi=hi, part=one) < 0 and b"adamw: the amax range must lie inside the buffer" in err()


def test_every_launching_entry_of_the_fourth_header_has_a_redzone_case():
    """the completeness check of tests/test_abi_arena_cpu.py, applied to include/t4r_hip_optim.h and tests/test_optim_clip_gpu.py"""
    import test_optim_clip_gpu as og

    exempt = {"t4r_grad_sumsq_parts": "size query: nothing launches"}
    names = _lib.header_symbols("t4r_hip_optim.h")
    cased = {e for c in og.REDZONE_CASES for e in c.entries}
    assert set(exempt) <= set(names)
    missing = [n for n in names if n not in cased and n not in exempt]
    assert not missing, f"entries of include/t4r_hip_optim.h with neither a red-zone case nor an exemption: {missing}"
    ids = [c.id for c in og.REDZONE_CASES]
    assert len(ids) == len(set(ids))


# ---------------------------------------------------------------------------------------------------------- schedules
def closed_form(name, w, T, cycles):
    """the lambdas of transformers.optimization.get_*_schedule_with_warmup, written out"""
    def f(s):
        if s < w:
            return s / max(1, w)
        if name == "constant_with_warmup":
            return 1.0
        if name == "linear":
            return max(0.0, (T - s) / max(1, T - w))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * cycles * 2.0 * (s - w) / max(1, T - w))))
    return f


def hf_multipliers(name, w, T, cycles, steps):
    """the learning rate a dummy SGD of lr 1 runs its steps at under the installed transformers scheduler; None if it has none"""
    try:
        from transformers import optimization as hf

        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=1.0)
        if name == "constant_with_warmup":
            sch = hf.get_constant_schedule_with_warmup(opt, num_warmup_steps=w)
        elif name == "linear":
            sch = hf.get_linear_schedule_with_warmup(opt, num_warmup_steps=w, num_training_steps=T)
        else:
            sch = hf.get_cosine_schedule_with_warmup(opt, num_warmup_steps=w, num_training_steps=T, num_cycles=cycles)
    except (ImportError, AttributeError):
        return None
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return out


@pytest.mark.parametrize("name", ["constant_with_warmup", "linear", "cosine"])
@pytest.mark.parametrize("w", [0, 7])
@pytest.mark.parametrize("cycles", [0.5, 2])
def test_warmup_schedule_equals_the_transformers_lambdas(name, w, cycles):
    T = 50
    f = optim.warmup_schedule(name, w, T, num_cycles=cycles)
    got = [f(s) for s in range(T)]
    want = hf_multipliers(name, w, T, cycles, T)
    if want is None:
        want = [closed_form(name, w, T, cycles)(s) for s in range(T)]
    assert len(got) == len(want) == 50
    assert max(abs(a - b) for a, b in zip(got, want)) <= 1e-12, (name, w, cycles)
    assert max(abs(a - closed_form(name, w, T, cycles)(s)) for s, a in enumerate(got)) <= 1e-12
    if w:
        assert got[0] == 0.0 and got[w] == 1.0
    with pytest.raises(ValueError):
        optim.warmup_schedule("polynomial", w, T)
    if name != "constant_with_warmup":
        with pytest.raises(ValueError):
            optim.warmup_schedule(name, w)


# ---------------------------------------------------------------------------------------------------------- FusedAdam on the host
def _flats():
    torch.manual_seed(0)
    lin = torch.nn.Linear(5, 3)
    emb = torch.nn.Embedding(11, 4)
    return optim.FlatParams(lin.named_parameters()), optim.FlatParams(emb.named_parameters())


def test_fused_adam_new_arguments_on_cpu_tensors():
    import inspect

    names = list(inspect.signature(optim.FusedAdam.__init__).parameters)
    assert names == ["self", "flats", "lr", "betas", "eps", "weight_decay", "max_grad_norm", "decoupled_weight_decay"]
    d = inspect.signature(optim.FusedAdam.__init__).parameters
    assert d["max_grad_norm"].default is None and d["decoupled_weight_decay"].default is False
    opt = optim.FusedAdam(_flats(), lr=2e-3, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0)
    assert opt.max_grad_norm == 1.0 and opt.decoupled_weight_decay is True and opt.last_grad_norm is None
    assert opt.set_schedule(optim.warmup_schedule("linear", 2, 6)) is opt
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.FusedAdam(_flats(), max_grad_norm=bad)
    # there is no CPU path: the clipped step refuses host tensors as every other op does, and so do the three ops
    with pytest.raises(_lib.T4RHipError):
        opt.step()
    g, part, out = torch.ones(8), torch.zeros(4, dtype=torch.float64), torch.zeros(2)
    with pytest.raises(_lib.T4RHipError):
        ops.grad_sumsq_(g, part)
    with pytest.raises(_lib.T4RHipError):
        ops.grad_clip_coef_(part, 1, 1.0, 1.0, out)
    with pytest.raises(_lib.T4RHipError):
        ops.adamw_step_(g, g.clone(), g.clone(), g.clone(), 1, decoupled=True, clip_coef=out[1:])


def test_fused_adam_state_dict_round_trip():
    opt = optim.FusedAdam(_flats(), lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05, decoupled_weight_decay=True,
                          max_grad_norm=0.5)
    g = torch.Generator().manual_seed(4)
    for m, v in opt.state:
        m.copy_(torch.randn(m.shape, generator=g))
        v.copy_(torch.rand(v.shape, generator=g))
    opt.step_count = 17
    sd = opt.state_dict()
    assert sd["step_count"] == 17 and len(sd["state"]) == 2
    assert sd["state"][0]["exp_avg"].data_ptr() != opt.state[0][0].data_ptr()             # copies, not views
    other = optim.FusedAdam(_flats())
    other.load_state_dict(sd)
    assert other.step_count == 17 and other.lr == other.base_lr == 2e-3 and other.betas == (0.8, 0.99) and other.eps == 1e-6
    assert other.weight_decay == 0.05 and other.decoupled_weight_decay is True and other.max_grad_norm == 0.5
    for (m, v), (m2, v2) in zip(opt.state, other.state):
        assert torch.equal(m, m2) and torch.equal(v, v2) and m.data_ptr() != m2.data_ptr()
    opt.state[0][0].zero_()                                                                # the dict does not alias the optimizer
    assert float(sd["state"][0]["exp_avg"].abs().max()) > 0
    torch.save(sd, os.devnull)                                                             # plain tensors and numbers
    with pytest.raises(ValueError):
        optim.FusedAdam(_flats()[:1]).load_state_dict(sd)


def test_documents_name_the_new_surface():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "125 entry points" in readme and "t4r_hip_optim.h" in readme and re.search(r"\b4 (optimizer )?entry points", readme)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "t4r_hip_optim.h" in integ and "decoupled_weight_decay=True" in integ and "max_grad_norm=1.0" in integ
    assert "warmup_schedule" in integ
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "grad_sumsq_kernel" in design and "grad_clip_coef_kernel" in design and "t4r_adamw_step" in design
