"""CPU: host side of the adjoint bilinear resample (``cmb_resample_bilinear_bwd``, elementwise.hip) — the binding, the
argument checks that run before anything is launched, and the ``CAMBRIAN_AMD_RESAMPLE_BWD`` switch.  No kernel is launched
here."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cambrian_amd import lib
    return lib


def test_symbol_is_bound_with_the_declared_signature(built):
    i32, i64, p = C.c_int32, C.c_int64, C.c_void_p
    want = (C.c_int, [C.c_int, p, i64, i32, i32, i64, i64, i64, p, i32, i32, i64, i64, p])
    assert built.SIGNATURES["cmb_resample_bilinear_bwd"] == want
    assert built.SIGNATURES["cmb_resample_bilinear_bwd"] == built.SIGNATURES["cmb_resample_bilinear"]   # the mirrored argument list
    fn = built.load().cmb_resample_bilinear_bwd
    assert fn.restype is C.c_int and list(fn.argtypes) == want[1]
    assert built.ABI_VERSION == 13 == built.load().cmb_abi_version()


def test_bad_arguments_are_rejected_before_any_launch(built):
    """Every case returns CMB_ERR_BAD_ARG from the host-side checks; the pointers are never dereferenced (this box may have
    no device at all)."""
    lib = built.load()
    bad, ok = -1, 0
    buf = (C.c_float * 16)()
    p = C.addressof(buf)

    def call(dtype=built.F32, dout=p, B=2, ho=6, wo=6, c=16, ld_dout=32, bs_dout=36 * 32, din=p, hi=4, wi=4, ld_din=16,
             bs_din=16 * 16):
        return lib.cmb_resample_bilinear_bwd(dtype, dout, B, ho, wo, c, ld_dout, bs_dout, din, hi, wi, ld_din, bs_din, None)

    assert call(c=12) == bad
    assert call(ld_dout=20) == bad
    assert call(din=None) == bad
    assert call(hi=0) == bad
    assert call(dout=None) == bad and call(ld_din=12) == bad and call(c=0) == bad and call(B=-1) == bad
    assert call(wi=0) == bad and call(ho=0) == bad and call(wo=-3) == bad
    assert call(B=0) == ok
    assert call(B=0, dtype=built.BF16) == ok


def test_switch_follows_the_environment(built, monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_RESAMPLE_BWD", raising=False)
    assert ops.resample_enabled()
    monkeypatch.setenv("CAMBRIAN_AMD_RESAMPLE_BWD", "0")
    assert not ops.resample_enabled()
    monkeypatch.setenv("CAMBRIAN_AMD_RESAMPLE_BWD", "1")
    assert ops.resample_enabled()


def test_supported_inputs_and_no_cpu_path(built, monkeypatch):
    from cambrian_amd import ops
    monkeypatch.delenv("CAMBRIAN_AMD_RESAMPLE_BWD", raising=False)
    assert ops.resample_supported(torch.bfloat16, 1152) and ops.resample_supported(torch.float32, 8)
    assert not ops.resample_supported(torch.float16, 64) and not ops.resample_supported(torch.bfloat16, 12)
    x = torch.zeros(2, 16, 8)
    assert ops.resample_bilinear(x, 4, 4, 4, 4) is x                    # equal grids: the input itself
    with pytest.raises(built.CambrianAmdError):
        ops.resample_bilinear(x, 4, 4, 6, 6)                            # the kernels have no CPU form
    with pytest.raises(built.CambrianAmdError):
        ops.resample_bilinear(x, 3, 3, 6, 6)                            # 16 rows are no 3 x 3 grid
