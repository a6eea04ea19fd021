"""CPU restatement of the MXFP4 format of ``cmb_quantize_mxfp4_rows`` / ``cmb_decode_linear_fp4`` in plain torch (no test in
this file): the quantiser and the dequantiser that every GPU kernel test of the format uses, so that the kernel tests do not
depend on the GPU quantiser, and that the GPU quantiser is compared with bit for bit.

Format: ``q`` uint8 [N, K / 2], byte j of a row = element 2 j in the low nibble, element 2 j + 1 in the high one; a nibble is an
OCP e2m1 code (bit 3 the sign, magnitudes ``GRID``); ``scales`` uint8 [N, K / 32], code c = 2^(c - 127).
Quantiser, per block of 32: amax = max |x|, e = clamp(floor(log2 amax) - 2, -126, 127), code e + 127 (a zero block: 127 and zero
nibbles); x 2^-e rounded to the grid, to nearest, ties to the even code, saturating at 6; what rounds to zero is written +0."""
import torch

BLOCK = 32
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# the midpoints between neighbouring grid values and whether the midpoint itself goes up (to the even code)
_MIDS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


def block_exponent(x: torch.Tensor) -> torch.Tensor:
    """e per block of 32 of x [N, K] (finite; fp32 or bf16): int32 [N, K / 32]; 0 for a zero block."""
    N, K = x.shape
    amax = x.float().abs().reshape(N, K // BLOCK, BLOCK).amax(-1)
    _, ex = torch.frexp(amax)                              # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = (ex.to(torch.int32) - 1 - 2).clamp(-126, 127)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def e2m1_codes(v: torch.Tensor) -> torch.Tensor:
    """fp32 values (already divided by the block scale) -> uint8 e2m1 codes, nearest, ties to even, saturating."""
    a = v.abs()
    code = torch.zeros_like(a, dtype=torch.int32)
    for mid, up in _MIDS:
        code += (a >= mid if up else a > mid).to(torch.int32)
    sign = ((v < 0) & (code > 0)).to(torch.int32) << 3
    return (code | sign).to(torch.uint8)


def quantize(x: torch.Tensor):
    """x [N, K] bf16 / fp32 on the CPU, finite, K % 32 == 0 -> (q uint8 [N, K / 2], scales uint8 [N, K / 32])."""
    N, K = x.shape
    assert K % BLOCK == 0 and K >= BLOCK
    e = block_exponent(x)
    inv = torch.ldexp(torch.ones((), dtype=torch.float32), -e)              # 2^-e: exact, normal for e in -126 .. 127
    v = x.float().reshape(N, K // BLOCK, BLOCK) * inv[..., None]            # an exact product (a power of two)
    codes = e2m1_codes(v).reshape(N, K)
    q = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return q.contiguous(), (e + 127).to(torch.uint8).contiguous()


def code_values(codes: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    grid = torch.tensor(GRID + tuple(-g for g in GRID), dtype=dtype)
    return grid[codes.long()]


def unpack(q: torch.Tensor) -> torch.Tensor:
    """uint8 [N, K / 2] -> e2m1 codes uint8 [N, K] in element order."""
    N, K2 = q.shape
    out = torch.empty(N, 2 * K2, dtype=torch.uint8)
    out[:, 0::2] = q & 15
    out[:, 1::2] = q >> 4
    return out


def pack(codes: torch.Tensor) -> torch.Tensor:
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def dequantize(q: torch.Tensor, scales: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """(q, scales) on the CPU -> the values [N, K] they stand for, exactly (float64 by default)."""
    N, K2 = q.shape
    vals = code_values(unpack(q.cpu()), dtype).reshape(N, 2 * K2 // BLOCK, BLOCK)
    scale = torch.ldexp(torch.ones((), dtype=dtype), scales.cpu().to(torch.int32) - 127)
    return (vals * scale[..., None]).reshape(N, 2 * K2)
