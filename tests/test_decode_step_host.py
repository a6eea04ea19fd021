"""CPU: host side of the one-call decode step (``cmb_decode_step`` / ``cmb_decode_step_ws``, decode_step.hip) and the greedy
selection between two steps (``cmb_decode_next``, decode_next.hip) — symbols and ABI revision, the argument checks that run
before anything is launched, the workspace total against the layout header, the opt-in switch, and the function that trims
a polled greedy loop back to where the per-token loop stops.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmb_decode_step", "cmb_decode_step_ws", "cmb_decode_next")
OK, BAD_ARG, ALIGNMENT, WORKSPACE = 0, -1, -2, -4


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_symbols_are_declared_exported_and_bound_under_revision_13(built):
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    lib = built.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in built.SIGNATURES
        assert getattr(lib, name).argtypes == built.SIGNATURES[name][1]       # resolves: the symbol left the library
        assert name in text[text.index("ABI revision"):text.index("#define CMB_ABI_VERSION")]
    assert built.ABI_VERSION == 13 == lib.cmb_abi_version()
    assert int(re.search(r"#define\s+CMB_ABI_VERSION\s+(\d+)", text).group(1)) == 13
    mk = open(os.path.join(ROOT, "cambrian_amd", "csrc", "Makefile")).read()
    assert "decode_step.hip" in mk and "decode_next.hip" in mk
    # the two descriptors: the binding's field lists are the header's, in order
    for struct, cls in (("cmb_decode_layer", built.DecodeLayer), ("cmb_decode_step_desc", built.DecodeStepDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *more = decl.split(",")
                fields += [re.search(r"(\w+)$", first.strip()).group(1)] + [m.strip() for m in more]
        assert fields == [f[0] for f in cls._fields_], struct


def _aligned(nbytes=256):
    raw = (C.c_char * (nbytes + 16))()
    return raw, (C.addressof(raw) + 15) & ~15


GEO = dict(B=3, H=256, I=512, nh=4, nkv=2, hd=64)


def _step_case(built, fp8=0, layers=2):
    """A well-formed argument set over a few host bytes (nothing is dereferenced on the device: every case below returns
    from the host-side checks, and the one complete set is never passed unchanged)."""
    keep, p = _aligned()
    table = (built.DecodeLayer * layers)()
    for row in table:
        for name, ld in (("qkv", 256), ("o", 256), ("gate_up", 256), ("down", 512)):
            setattr(row, "w_" + name, p)
            setattr(row, "ld_" + name, ld)
            setattr(row, "w_" + name + "_scale", p if fp8 else None)
        row.norm1 = row.norm2 = row.kcache = row.vcache = p
    desc = built.DecodeStepDesc(layers=layers, fp8=fp8, V=64, eps=1e-5, scale=0.125, c_sb=2 * 64 * 64, c_sh=64 * 64, c_st=64,
                                final_norm=p, head=p, ld_head=256, head_scale=p if fp8 else None, **GEO)
    return keep, p, desc, table


def test_step_rejects_bad_arguments_before_any_launch(built):
    lib = built.load()
    for fp8 in (0, 1):
        keep, p, desc, table = _step_case(built, fp8)
        t = 36
        need = lib.cmb_decode_step_ws(*GEO.values(), t)
        assert need > 0

        def call(d=desc, tab=table, x=p + (1 << 20), x_ld=256, cos=p, sin=p, t=t, kv=p, kv_ld=64, ws=p, ws_floats=need - 1,
                 logits=p, l_ld=64):
            d = None if d is None else C.byref(d)
            return lib.cmb_decode_step(d, tab, x, x_ld, cos, sin, t, kv, kv_ld, ws, ws_floats, logits, l_ld, None)

        # the reference point of this test: everything in order but the workspace, one float short
        assert call() == WORKSPACE
        assert call(ws_floats=0) == WORKSPACE
        assert call(d=None) == BAD_ARG and call(tab=None) == BAD_ARG
        for name in ("x", "cos", "sin", "kv", "ws", "logits"):
            assert call(**{name: None}) == BAD_ARG, f"NULL {name}"

        def with_desc(ws_floats=need - 1, **over):
            _, _, d2, _ = _step_case(built, fp8)
            for k, v in over.items():
                setattr(d2, k, v)
            return call(d=d2, ws_floats=ws_floats)

        assert with_desc(layers=0) == BAD_ARG and with_desc(layers=-1) == BAD_ARG
        assert with_desc(B=0) == BAD_ARG and with_desc(B=17) == BAD_ARG and with_desc(B=-1) == BAD_ARG
        assert with_desc(B=16, ws_floats=0) == WORKSPACE and with_desc(B=1, ws_floats=0) == WORKSPACE   # the range's ends are taken
        assert with_desc(hd=80) == BAD_ARG and with_desc(nh=3) == BAD_ARG and with_desc(H=260) == BAD_ARG
        assert with_desc(V=0) == BAD_ARG and with_desc(eps=-1.0) == BAD_ARG
        assert with_desc(final_norm=None) == BAD_ARG and with_desc(head=None) == BAD_ARG
        assert with_desc(ld_head=248) == BAD_ARG and with_desc(ld_head=260) == BAD_ARG
        assert call(t=-1) == BAD_ARG and call(kv_ld=t) == BAD_ARG
        assert call(x_ld=248) == BAD_ARG and call(x_ld=260) == BAD_ARG and call(l_ld=60) == BAD_ARG and call(l_ld=68) == BAD_ARG
        assert call(x=p, ws_floats=need) == BAD_ARG                                  # x inside the workspace
        # a misaligned pointer, wherever it is
        for name in ("x", "ws", "logits"):
            assert call(**{name: p + (1 << 20) + 4}) == ALIGNMENT, f"misaligned {name}"
        assert with_desc(final_norm=p + 8) == ALIGNMENT and with_desc(head=p + 2) == ALIGNMENT
        assert with_desc(c_st=68) == ALIGNMENT and with_desc(c_sh=4100) == ALIGNMENT
        for field in ("w_qkv", "w_o", "w_gate_up", "w_down", "norm1", "norm2", "kcache", "vcache"):
            _, _, _, tab = _step_case(built, fp8)
            setattr(tab[1], field, p + 8)
            assert call(tab=tab) == ALIGNMENT, field
            setattr(tab[1], field, None)
            assert call(tab=tab) == BAD_ARG, field
        _, _, _, tab = _step_case(built, fp8)
        tab[0].ld_down = 504
        assert call(tab=tab) == BAD_ARG
        if fp8:
            _, _, _, tab = _step_case(built, fp8)
            tab[1].w_o_scale = None
            assert call(tab=tab) == BAD_ARG
            tab[1].w_o_scale = p + 2
            assert call(tab=tab) == ALIGNMENT
            assert with_desc(head_scale=None) == BAD_ARG
            assert with_desc(H=264) == BAD_ARG           # K % 16 for the 1-byte weights (264 is fine for bf16's K % 8)
        del keep


def test_next_rejects_bad_arguments_before_any_launch(built):
    lib = built.load()
    keep, p = _aligned()

    def call(logits=p, l_ld=64, B=3, V=64, eos=-1, done=p, out=p, out_ld=8, step=0, n_tok=p, pos=p, kv=p, kv_ld=64, t=36,
             embed=p, e_ld=256, rows=64, H=256, x=p, x_ld=256, hd=64, base=1e4, cos=p, sin=p):
        return lib.cmb_decode_next(logits, l_ld, B, V, eos, done, out, out_ld, step, n_tok, pos, kv, kv_ld, t, embed, e_ld, rows,
                                   H, x, x_ld, hd, base, cos, sin, None)

    for name in ("logits", "out", "n_tok", "pos", "kv", "embed", "x", "cos", "sin"):
        assert call(**{name: None}) == BAD_ARG, f"NULL {name}"
    assert call(done=None, eos=5) == BAD_ARG                      # an eos id needs the done flags
    assert call(B=0) == BAD_ARG and call(B=17) == BAD_ARG
    assert call(V=0) == BAD_ARG and call(V=1 << 31) == BAD_ARG and call(l_ld=63) == BAD_ARG
    assert call(rows=63) == BAD_ARG and call(eos=64) == BAD_ARG and call(eos=-2) == BAD_ARG
    assert call(step=-1) == BAD_ARG and call(step=8) == BAD_ARG and call(t=-1) == BAD_ARG and call(t=64) == BAD_ARG
    assert call(H=252) == BAD_ARG and call(H=0) == BAD_ARG and call(e_ld=248) == BAD_ARG and call(x_ld=260) == BAD_ARG
    assert call(hd=63) == BAD_ARG and call(hd=0) == BAD_ARG
    assert call(embed=p + 8) == ALIGNMENT and call(x=p + 2) == ALIGNMENT and call(logits=p + 2) == ALIGNMENT
    assert call(out=p + 4) == ALIGNMENT and call(pos=p + 4) == ALIGNMENT
    del keep


def test_workspace_total_is_the_layout_headers(built, tmp_path):
    """``cmb_decode_step_ws`` against ``dsl_make(...).total`` of csrc/decode_step_layout.h, evaluated by the layout sim
    (plain g++ here; tests/test_decode_step_layout_sim.py runs the same program's full check under the sanitizers)."""
    lib = built.load()
    exe = str(tmp_path / "sim")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "csrc", "decode_step_layout_sim.cpp"), "-o", exe],
                   check=True)
    cases = []
    for B in (1, 2, 3, 5, 16):
        for H, I, nh, nkv, hd in ((256, 512, 4, 2, 64), (264, 520, 4, 4, 64), (384, 1000, 4, 1, 96), (4096, 14336, 32, 8, 128)):
            for t in (0, 36, 299, 2048, 5000):
                attn = lib.cmb_decode_attn_ws(B, nh, nkv, hd, t, 0)
                assert attn >= 0
                cases.append(((B, H, I, nh, nkv, hd, t), attn))
    assert any(a > 0 for _, a in cases) and any(a == 0 for _, a in cases)      # split and unsplit plans are both in the grid
    args = [str(v) for (B, H, I, nh, nkv, hd, t), attn in cases for v in (B, H, I, nh, nkv, hd, attn)]
    out = subprocess.run([exe, "--total"] + args, capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(cases)
    for (geo, _), want in zip(cases, out):
        assert lib.cmb_decode_step_ws(*geo) == int(want), geo
    # non-decreasing in t_max: a workspace sized at the largest t of a call serves every step
    for B in (1, 4, 16):
        sizes = [lib.cmb_decode_step_ws(B, 4096, 14336, 32, 8, 128, t) for t in range(0, 6000, 97)]
        assert sizes == sorted(sizes)
    assert lib.cmb_decode_step_ws(0, 256, 512, 4, 2, 64, 3) == BAD_ARG and lib.cmb_decode_step_ws(17, 256, 512, 4, 2, 64, 3) == BAD_ARG
    assert lib.cmb_decode_step_ws(1, 256, 512, 4, 2, 80, 3) == BAD_ARG and lib.cmb_decode_step_ws(1, 256, 512, 4, 2, 64, -1) == BAD_ARG


def test_switch_env_over_config_default_off(built, monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_STEP", raising=False)
    assert ops.decode_step_enabled() is False                      # default off
    assert ops.decode_step_enabled(False) is False and ops.decode_step_enabled(True) is True
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", "1")
    assert ops.decode_step_enabled() and ops.decode_step_enabled(False) and ops.decode_step_enabled(True)
    monkeypatch.setenv("CAMBRIAN_AMD_DECODE_STEP", "0")
    assert not ops.decode_step_enabled() and not ops.decode_step_enabled(True)      # the environment overrides the config
    monkeypatch.delenv("CAMBRIAN_AMD_DECODE_FP8", raising=False)
    assert ops.decode_fp8_enabled() is False                       # the fp8 switch is its own
    assert ops.DECODE_STEP_POLL == 8
    from cambrian_amd.model.language_model.cambrian_llama import llama3_8b_config
    assert not getattr(llama3_8b_config(), "decode_step_fused", False)              # absent from the config = off


def _per_token_loop(ids: torch.Tensor, eos: int) -> torch.Tensor:
    """The per-token greedy loop of ``generate()`` replayed on the tokens it would have chosen: stop after the first step at
    which every row is done (a row is done from its first eos on), or at the end."""
    B, n = ids.shape
    done = torch.zeros(B, dtype=torch.bool)
    out = []
    for step in range(n):
        nxt = ids[:, step]
        assert bool((nxt[done] == eos).all()), "the planted matrix is not one a greedy loop can produce"
        done = done | (nxt == eos)
        out.append(nxt)
        if step + 1 == n or bool(done.all()):
            break
    return torch.stack(out, 1)


def _planted(gen, B, n, eos, first_eos):
    """Random ids without eos, then row b emits eos from column first_eos[b] on (None: never), as the device loop does."""
    ids = torch.randint(0, 50, (B, n), generator=gen)
    ids[ids == eos] = eos + 1
    for b, c in enumerate(first_eos):
        if c is not None:
            ids[b, c:] = eos
    return ids


@pytest.mark.parametrize("first_eos", [
    (5, 11, 3),            # all rows done at step 11: not a multiple of 8
    (8, 2, 8),             # at step 8
    (7, 7, 0),             # at step 7, the column the first poll looks at (and a row done at step 0)
    (None, 4, 9),          # never: one row goes on to the end
    (None, None, None),    # never, no eos at all
    (0, 0, 0),             # every row done at step 0
    (0, 13, 6),            # a row that is done at step 0
    (23, 1, 2),            # the last column
])
def test_trim_equals_the_per_token_loop(built, first_eos):
    from cambrian_amd import ops
    gen = torch.Generator().manual_seed(sum(7 * (c or 1) for c in first_eos))
    eos, n = 7, 24
    ids = _planted(gen, len(first_eos), n, eos, first_eos)
    want = _per_token_loop(ids, eos)
    # the polled loop hands the trim what it has produced when it stops: at a poll boundary past the stopping column, or all
    stops = [c for c in range(want.shape[1], n + 1) if c % ops.DECODE_STEP_POLL == 0 or c == n]
    for upto in (stops[0], n):
        got = ops.trim_after_all_done(ids[:, :upto], eos)
        assert torch.equal(got, want), (first_eos, upto)
    if all(c is not None for c in first_eos):
        assert want.shape[1] == max(first_eos) + 1
    else:
        assert want.shape[1] == n
    assert ops.trim_after_all_done(ids[:, :0], eos).shape == (len(first_eos), 0)
