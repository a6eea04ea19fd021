"""CPU: host side of the commuted aux projection — ``cmb_resample_accum`` in the header, the export map and the binding (ABI
revision unchanged), its argument checks (which run before any launch), the stage plan of ``ops.linear_stage_maps``, the
switch, and which towers offer stage maps.  No kernel is launched here."""
import ctypes as C
import fnmatch
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_header_export_map_and_binding_carry_the_kernel(built):
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    assert re.search(r"\bint\s+cmb_resample_accum\s*\(\s*const\s+cmb_resample_accum_desc\s*\*", text)
    assert int(re.search(r"#define\s+CMB_RESAMPLE_ACCUM_MAX_SRC\s+(\d+)", text).group(1)) == built.RESAMPLE_ACCUM_MAX_SRC == 4
    # the version script exports by pattern: the name must match a global pattern, and the built library must export it
    vs = open(os.path.join(ROOT, "cambrian_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:(.*?)local:", re.sub(r"/\*.*?\*/", "", vs, flags=re.S), flags=re.S).group(1)
    assert any(fnmatch.fnmatchcase("cmb_resample_accum", g.strip()) for g in globs.split(";") if g.strip())
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "cmb_resample_accum" in [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert built.SIGNATURES["cmb_resample_accum"] == (C.c_int, [C.POINTER(built.ResampleAccumDesc), C.c_void_p])
    fn = built.load().cmb_resample_accum
    assert fn.restype is C.c_int
    # added under the current revision: nothing that existed changed
    assert built.ABI_VERSION == 13 == built.load().cmb_abi_version()
    assert int(re.search(r"#define\s+CMB_ABI_VERSION\s+(\d+)", text).group(1)) == 13


def test_descriptor_layout_matches_the_header(built):
    """Field order and types of the ctypes mirror against the struct text of the header."""
    text = open(os.path.join(ROOT, "include", "cambrian_amd.h")).read()
    body = re.search(r"typedef struct cmb_resample_accum_desc \{(.*?)\} cmb_resample_accum_desc;", text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            decl = re.sub(r"^(const\s+)?(void|float|int32_t|int64_t)\s*\*?", "", decl)
            names += [re.sub(r"\[.*?\]|\*|\s", "", n) for n in decl.split(",")]
    assert names == [f[0] for f in built.ResampleAccumDesc._fields_]
    assert C.sizeof(built.ResampleAccumDesc) == 16 + 8 + 8 + 8 + 24 + 8 + 32 + 32 + 64 + 24 + 24


def test_bad_arguments_are_rejected_before_any_launch(built):
    """The pointers are never dereferenced (this box may have no device at all)."""
    lib = built.load()
    ok, bad, align = 0, -1, -2
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16

    def call(**kw):
        d = built.ResampleAccumDesc()
        d.dtype, d.src_dtype, d.act, d.n_src = built.F32, built.F32, built.ACT_GELU_ERF, 1
        d.B, d.Ho, d.Wo, d.C = 2, 6, 6, 16
        d.base, d.ld_base, d.batch_stride_base = p, 16, 36 * 16
        d.bias = p
        d.src[0], d.Hi[0], d.Wi[0], d.ld_src[0], d.batch_stride_src[0] = p, 4, 4, 16, 16 * 16
        d.pre_out, d.ld_pre, d.batch_stride_pre = p, 16, 36 * 16
        d.out, d.ld_out, d.batch_stride_out = p, 32, 36 * 32
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return lib.cmb_resample_accum(C.byref(d), None)

    assert call(B=0) == ok                                   # everything valid, nothing to do
    assert call(out=None) == bad                             # NULL out
    assert call(C=12) == bad
    assert call(n_src=5) == bad and call(n_src=-1) == bad
    assert call(act=7) == bad and call(act=built.ACT_SILU) == bad
    assert call(out=p + 4) == align                          # a misaligned pointer
    assert call(base=p + 8) == align and call(bias=p + 4) == align and call(src=(0, p + 4)) == align and call(pre_out=p + 2) == align
    assert call(ld_out=20) == bad and call(ld_base=12) == bad and call(ld_src=(0, 12)) == bad and call(batch_stride_pre=4) == bad
    assert call(ld_out=8) == bad                             # rows narrower than C
    assert call(src=(0, None)) == bad and call(Hi=(0, 0)) == bad and call(Wo=0) == bad and call(B=-1) == bad
    assert call(n_src=0, base=None) == bad                   # nothing to sum
    assert call(n_src=0, B=0) == ok and call(base=None, bias=None, pre_out=None, B=0) == ok
    # dtype pairs: bf16 | bf16, fp32 | fp32, fp32 partial products under a bf16 output — and nothing else
    assert call(dtype=built.BF16, src_dtype=built.BF16, B=0) == ok and call(dtype=built.BF16, src_dtype=built.F32, B=0) == ok
    assert call(dtype=built.F32, src_dtype=built.BF16, B=0) == bad and call(dtype=built.F16, B=0) == bad
    assert call(src_dtype=built.FP8_E4M3, B=0) == bad
    assert call(n_src=4, src=(3, None), B=0) == bad          # every listed source is checked


def test_stage_plan(built):
    from cambrian_amd import ops
    assert ops.stage_maps_plan([256, 128, 64, 32], 96) == [False, False, True, True]
    assert ops.stage_maps_plan([16, 8, 4, 2], 8) == [False, False, True, True]
    assert ops.stage_maps_plan([8], 8) == [False]                                   # an equal grid is dense
    assert ops.stage_maps_plan([(4, 6), (7, 3), (5, 5)], 5) == [True, True, False]  # positions decide, not sides
    assert ops.stage_maps_plan([32, 16, 8, 4], 12) == [False, False, True, True]
    assert ops.stage_maps_plan([], 4) == []


def test_switch_is_off_by_default_and_follows_environment_and_config(built, monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_COMMUTED_PROJ", raising=False)
    assert not ops.commuted_proj_enabled() and not ops.commuted_proj_enabled(SimpleNamespace())
    assert ops.commuted_proj_enabled(SimpleNamespace(mm_commuted_aux_projection=True))
    assert not ops.commuted_proj_enabled(SimpleNamespace(mm_commuted_aux_projection=False))
    monkeypatch.setenv("CAMBRIAN_AMD_COMMUTED_PROJ", "1")
    assert ops.commuted_proj_enabled() and ops.commuted_proj_enabled(SimpleNamespace(mm_commuted_aux_projection=False))
    monkeypatch.setenv("CAMBRIAN_AMD_COMMUTED_PROJ", "0")
    assert not ops.commuted_proj_enabled()


def test_cpu_inputs_are_not_fusable_and_there_is_no_cpu_path(built, monkeypatch):
    from cambrian_amd import ops
    monkeypatch.setenv("CAMBRIAN_AMD_COMMUTED_PROJ", "1")
    maps = [torch.zeros(1, s, s, 64) for s in (8, 2)]
    w = torch.zeros(64, 128)
    assert not ops.stage_maps_fusable(maps, 4, w, None, built.ACT_NONE)
    with pytest.raises(built.CambrianAmdError):
        ops.linear_stage_maps(maps, 4, w)                    # the unfused composition has no CPU form either
    with pytest.raises(built.CambrianAmdError):
        ops.k_resample_accum(torch.zeros(1, 16, 8), 4, 4, base=torch.zeros(1, 16, 8))


def test_stage_maps_holder():
    from cambrian_amd import ops
    sm = ops.StageMaps([torch.zeros(2, 16, 16, 64, dtype=torch.bfloat16), torch.zeros(2, 4, 4, 128, dtype=torch.bfloat16)], 8)
    assert sm.shape == (2, 64, 192) and sm.shape[1] == 64 and sm.dtype == torch.bfloat16 and sm.device.type == "cpu"
    assert not sm.requires_grad and sm.side == 8 and len(sm.maps) == 2


def test_only_multi_stage_towers_with_an_interp_size_offer_stage_maps():
    from cambrian_amd.model.multimodal_encoder.clip_convnext_encoder import CLIPConvNextTower
    args = SimpleNamespace()
    offers = {n: CLIPConvNextTower(n, args, delay_load=True).offers_stage_maps
              for n in ("clip-convnext-XXL-multi-stage-res1024-interp9216", "clip-convnext-L-multi-stage-res256-interp144",
                        "clip-convnext-XXL-multi-stage", "clip-convnext-L-res256-interp144", "clip-convnext-L")}
    assert offers == {"clip-convnext-XXL-multi-stage-res1024-interp9216": True,
                      "clip-convnext-L-multi-stage-res256-interp144": True,
                      "clip-convnext-XXL-multi-stage": False, "clip-convnext-L-res256-interp144": False,
                      "clip-convnext-L": False}
    t = CLIPConvNextTower("clip-convnext-XXL-multi-stage", args, delay_load=True)
    assert t.forward_stage_maps(torch.zeros(1, 3, 64, 64)) is None        # nothing to offer: the caller takes forward()
    t = CLIPConvNextTower("clip-convnext-XXL-multi-stage-res1024-interp9216", args, delay_load=True)
    assert t.forward_stage_maps([torch.zeros(3, 64, 64)]) is None         # per-sample lists keep the ordinary path
