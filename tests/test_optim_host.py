"""CPU: the optimizer entry points (cmb_optim_chunks, cmb_grad_sqnorm, cmb_grad_sqnorm_workspace, cmb_adamw_step) are declared,
exported and bound under the unchanged ABI revision; their host-side checks answer before anything is launched; FusedAdamW
refuses what it does not implement.  No kernel runs here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("cmb_optim_chunks", "cmb_grad_sqnorm_workspace", "cmb_grad_sqnorm", "cmb_adamw_step")
OK, BAD_ARG, WORKSPACE = 0, -1, -4


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_symbols_declared_exported_bound_abi_unchanged(built):
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = built.load()
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} is not declared in cambrian_amd.h"
        assert hasattr(lib, s) and s in built.SIGNATURES
    assert "cmb_optim_job" in code
    assert built.ABI_VERSION == 13 == lib.cmb_abi_version()
    assert int(re.search(r"#define\s+CMB_ABI_VERSION\s+(\d+)", text).group(1)) == 13
    # the ctypes mirror has the C struct's size: 5 pointers, 2 int64, 2 int32
    assert C.sizeof(built.OptimJob) == 64


def test_chunk_count(built):
    from cambrian_amd import ops
    lib = built.load()
    chunk = ops.OPTIM_CHUNK
    assert chunk & (chunk - 1) == 0 and chunk <= 65536
    assert lib.cmb_optim_chunks(0) == 0 and lib.cmb_optim_chunks(-5) == 0
    assert lib.cmb_optim_chunks(chunk) == 1 and lib.cmb_optim_chunks(chunk + 1) == 2   # ops.OPTIM_CHUNK is the library's
    prev = 0
    for n in (1, 7, 8, 9, 4095, 4096, 4097, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 10 ** 9 + 7, 2 ** 40 + 1):
        k = lib.cmb_optim_chunks(n)
        assert k >= prev, "not monotone"
        assert k * chunk >= n > (k - 1) * chunk
        prev = k


def test_workspace_query(built):
    lib = built.load()
    assert lib.cmb_grad_sqnorm_workspace(0) == 0 and lib.cmb_grad_sqnorm_workspace(-3) == 0
    assert lib.cmb_grad_sqnorm_workspace(1) == 1 and lib.cmb_grad_sqnorm_workspace(12345) == 12345
    assert lib.cmb_grad_sqnorm_workspace(2 ** 33) == 2 ** 33


def test_bad_arguments_answer_before_any_launch(built):
    """Every call below must return from the host-side checks: this machine may have no device at all, and a launch would
    answer CMB_ERR_LAUNCH (or worse) instead."""
    lib = built.load()
    tab, ws, out = 0x1000, 0x2000, 0x3000   # never dereferenced on the host
    sq = lib.cmb_grad_sqnorm
    assert sq(None, 1, 1, ws, 1, out, None) == BAD_ARG            # no table for one job
    assert sq(tab, -1, 0, ws, 1, out, None) == BAD_ARG            # negative job count
    assert sq(tab, 1, -1, ws, 1, out, None) == BAD_ARG            # negative chunk count
    assert sq(None, 0, 3, ws, 3, out, None) == BAD_ARG            # chunks of no tensor
    assert sq(tab, 1, 1, ws, 1, None, None) == BAD_ARG            # nowhere to put the result
    assert sq(tab, 1, 1, None, 1, out, None) == BAD_ARG           # no workspace for one chunk
    assert sq(tab, 1, 1, ws, -1, out, None) == BAD_ARG            # negative workspace size
    assert sq(tab, 2, 5, ws, 4, out, None) == WORKSPACE           # one float short
    assert sq(tab, 2, 5, ws, 0, out, None) == WORKSPACE
    st = lib.cmb_adamw_step
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 1.0)          # lr, betas, eps, wd, bias corrections, grad_scale
    assert st(None, 1, 1, *hp, None, 0.0, None) == BAD_ARG
    assert st(tab, -1, 0, *hp, None, 0.0, None) == BAD_ARG
    assert st(tab, 1, -2, *hp, None, 0.0, None) == BAD_ARG
    assert st(None, 0, 1, *hp, None, 0.0, None) == BAD_ARG
    assert st(tab, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.001, 1.0, None, 0.0, None) == BAD_ARG    # bias_correction1 = 0
    assert st(tab, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, -1.0, 1.0, None, 0.0, None) == BAD_ARG     # bias_correction2 < 0
    assert st(tab, 1, 1, float("nan"), 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 1.0, None, 0.0, None) == BAD_ARG
    assert st(tab, 1, 1, 1e-3, 0.9, 0.999, -1e-8, 0.0, 0.1, 0.001, 1.0, None, 0.0, None) == BAD_ARG   # negative eps
    # nothing to do is not an error, and launches nothing: an empty table, and jobs that are all empty tensors
    assert st(None, 0, 0, *hp, None, 0.0, None) == OK
    assert st(tab, 3, 0, *hp, None, 1.0, None) == OK


def test_ops_refuse_cpu_tensors(built):
    from cambrian_amd import ops
    g = torch.ones(8)
    with pytest.raises(built.CambrianAmdError):
        ops.grad_sqnorm([g])
    with pytest.raises(built.CambrianAmdError):
        ops.adamw_step([g], [g.clone()], [g.clone()], [g.clone()], lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                       weight_decay=0.0, step=1)


def test_fused_adamw_refuses_what_it_does_not_implement(built):
    from cambrian_amd.train.fused_adamw import FusedAdamW
    p = torch.nn.Parameter(torch.ones(8))
    with pytest.raises(ValueError, match="ROCm device"):
        FusedAdamW([p], lr=1e-3)
    with pytest.raises(ValueError, match="ROCm device"):
        FusedAdamW([{"params": [p], "lr": 1e-4}], lr=1e-3)
    for mode in ("amsgrad", "maximize", "capturable"):
        with pytest.raises(ValueError, match=mode):
            FusedAdamW([p], lr=1e-3, **{mode: True})
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW([{"params": [p], "amsgrad": True}], lr=1e-3)
    with pytest.raises(ValueError):
        FusedAdamW([p], lr=1e-3, max_grad_norm=0.0)
    with pytest.raises(ValueError):
        FusedAdamW([], lr=1e-3)
    # a closure is refused before anything else happens in step(): an optimizer without stepped tensors shows it on a CPU
    opt = FusedAdamW([torch.nn.Parameter(torch.ones(2), requires_grad=False)], lr=1e-3)
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)
    assert opt.step() is None and opt.last_grad_norm is None
