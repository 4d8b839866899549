"""Strided placements of a logical [N, L, H, dh] tensor for the tests of the view-taking C entry points
(include/ampconv.h: ampconv_view_t), and the guard bytes around them.

TEST INFRASTRUCTURE.  `place` puts a logical tensor into ONE allocation under one of the LAYOUTS below, with a margin
in front of and behind the view's extent and, for the padded layouts, gaps inside it:
  * an INPUT buffer holds NaN everywhere outside the view: a kernel that lets a byte of a gap or margin reach a result
    (an over-read, a stride ignored, a padding lane zeroed by multiplying with 0) shows up as NaN;
  * an OUTPUT buffer holds a sentinel bit pattern everywhere: afterwards every element outside the view must still be the
    sentinel, every element inside must have been overwritten (`outside_intact`, `unwritten`).
The margins also keep a stray access inside memory the test owns.  tools/bench_kernels.py --layout= times the same stride
triples (`layout_strides`).
"""
import numpy as np
import torch

from ampnet_amd import _lib

# id -> (node, row, head) stride in elements, D = H * dh; see layout_strides for the bases
LAYOUTS = ('nld', 'packed3', 'nhld', 'hnld', 'lnd', 'pad16', 'pad8', 'pad4')
# 'mixed': every operand in another layout (the alignment class of a call is the minimum over its views)
MIXED = {'Q': 'nhld', 'K': 'packed3', 'V': 'hnld', 'dO': 'pad16', 'out0': 'lnd', 'out1': 'pad16'}
# quiet-NaN patterns no kernel produces (fp32: hip's NaN is 0x7FC00000; bf16: 0x7FC0)
SENTINEL = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FA5}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
# integer buffers (place_flat_int): outputs hold a pattern no index, count or offset of a test reaches; the margins of an
# input hold -1, the one value that, taken for an index, count or pointer by a stray read, addresses nothing outside
# the allocation's own margins
SENTINEL.update({torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A})
_INT.update({torch.int32: torch.int32, torch.int64: torch.int64})
INT_POISON = -1


def layout_strides(layout, N, L, H, dh, bf16=False):
    """(node_stride, row_stride, head_stride, base offset) in elements.  The base offset counts from a 256-byte aligned
    origin: D for the K third of a packed projection, the misalignment itself for pad8 / pad4."""
    D = H * dh
    e = 2 if bf16 else 1                      # elements per 4 bytes
    if layout == 'nld':                       # canonical row-major [N, L, D]
        return L * D, D, dh, 0
    if layout == 'packed3':                   # the K third of a packed [N * L, 3 D] projection: what ships
        return 3 * L * D, 3 * D, dh, D
    if layout == 'nhld':                      # a contiguous [L, dh] tile per (node, head)
        return H * L * dh, dh, L * dh, 0
    if layout == 'hnld':                      # head-outermost
        return L * dh, dh, N * L * dh, 0
    if layout == 'lnd':                       # token-outermost
        return D, N * D, dh, 0
    if layout == 'pad16':                     # 16-byte gaps behind every row, two empty rows behind every node
        row = D + 4 * e
        return (L + 2) * row, row, dh, 0
    if layout == 'padrow':                    # 16-byte gaps behind every row only (a row-major matrix with a leading dimension)
        row = D + 4 * e
        return L * row, row, dh, 0
    if layout == 'pad8':                      # 8-byte gaps, base 8 bytes off: 8-byte alignment only
        row = D + 2 * e
        return L * row, row, dh, 2 * e
    if layout == 'pad4':                      # fp32: 4-byte gaps, base 4 bytes off: 4-byte alignment only
        assert not bf16
        return L * (D + 1), D + 1, dh, 1
    raise ValueError(layout)


def alignment_bytes(views, esize):
    """The largest power of two (at most 16) that divides every base address and every stride, in bytes."""
    a = 16
    for v in views:
        for x in (v.ptr, v.node_stride * esize, v.row_stride * esize, v.head_stride * esize):
            while x % a:
                a //= 2
    return a


class Placed:
    """backing: the one allocation; view: the _lib.View into it; index: [N, L, H, dh] int64 positions in `backing`."""

    def __init__(self, backing, view, index):
        self.backing, self.view, self.index = backing, view, index

    def __iter__(self):                       # backing, view, index = place(...)
        return iter((self.backing, self.view, self.index))

    def bits(self):
        return self.backing.view(_INT[self.backing.dtype])

    def outside_intact(self, rows=None):
        """True iff every element outside the view -- and, with `rows`, outside those nodes of it -- is the sentinel."""
        inside = torch.zeros(self.backing.numel(), dtype=torch.bool, device=self.backing.device)
        inside[(self.index if rows is None else self.index[rows]).reshape(-1)] = True
        return bool((self.bits()[~inside] == _sentinel(self.backing.dtype)).all())

    def margins_hold(self, value):
        """True iff every element outside the buffer still holds `value` (NaN: is NaN) -- for an INPUT the call also
        writes (its margins hold NaN or INT_POISON, not the sentinel)."""
        inside = torch.zeros(self.backing.numel(), dtype=torch.bool, device=self.backing.device)
        inside[self.index.reshape(-1)] = True
        out = self.backing[~inside]
        return bool(torch.isnan(out).all() if value != value else (out == value).all())

    def unwritten(self, rows=None):
        """Number of elements of the view (of those nodes) that still hold the sentinel."""
        idx = (self.index if rows is None else self.index[rows]).reshape(-1)
        return int((self.bits()[idx] == _sentinel(self.backing.dtype)).sum())


def _sentinel(dtype):
    s = SENTINEL[dtype]
    return s - (1 << 16) if dtype == torch.bfloat16 and s >= (1 << 15) else s


def place(logical, layout, dtype, role, device='cuda:0'):
    """logical: an array [N, L, H, dh] -> an INPUT buffer (NaN around the values; float32 arrays are placed bit for bit),
    or that shape as a tuple -> an OUTPUT buffer full of the sentinel.  role ('Q', 'K', 'V', 'dO', 'out0', 'out1') picks
    the operand's layout under 'mixed'.  Returns a Placed; `backing, view, index = place(...)` unpacks it."""
    is_output = isinstance(logical, tuple)
    N, L, H, dh = logical if is_output else logical.shape
    if layout == 'mixed':
        layout = MIXED[role]
    bf16 = dtype == torch.bfloat16
    ns, rs, hs, off = layout_strides(layout, N, L, H, dh, bf16)
    span = (N - 1) * ns + (L - 1) * rs + (H - 1) * hs + dh
    margin = -(-(max(ns, rs, hs) + L * H * dh) // 64) * 64           # >= one node's extent, a whole number of 128 bytes
    n, l, h, c = np.ix_(np.arange(N) * ns, np.arange(L) * rs, np.arange(H) * hs, np.arange(dh))
    index = torch.from_numpy(margin + off + n + l + h + c).to(device)
    total = margin + off + span + margin
    if is_output:
        backing = torch.full((total,), _sentinel(dtype), dtype=_INT[dtype], device=device).view(dtype)
    else:
        backing = torch.full((total,), float('nan'), dtype=dtype, device=device)
        vals = torch.from_numpy(np.ascontiguousarray(logical))
        backing[index.reshape(-1)] = vals.to(dtype).to(device).reshape(-1)          # (float32 -> float32: bit for bit)
    assert backing.data_ptr() % 64 == 0
    view = _lib.View(backing.data_ptr() + (margin + off) * backing.element_size(), ns, rs, hs)
    return Placed(backing, view, index)


def place_flat(logical, dtype, skew=0, device='cuda:0'):
    """`place` for the calls that take a plain pointer: logical, an array of any shape, -> a contiguous INPUT buffer inside
    a larger allocation with NaN in front of and behind it (float32 arrays are placed bit for bit); that shape as a tuple
    -> an OUTPUT buffer, the whole allocation full of the sentinel.  The buffer begins `skew` elements behind a 256-byte
    boundary.  Returns a Placed whose `ptr` is the buffer's address (`view`: None)."""
    is_output = isinstance(logical, tuple)
    shape = logical if is_output else logical.shape
    n = int(np.prod(shape, dtype=np.int64))
    margin = 64 * (1 + skew // 64) + 64
    total = margin + skew + n + 64
    if is_output:
        backing = torch.full((total,), _sentinel(dtype), dtype=_INT[dtype], device=device).view(dtype)
    else:
        backing = torch.full((total,), float('nan'), dtype=dtype, device=device)
        vals = torch.from_numpy(np.ascontiguousarray(logical))
        backing[margin + skew:margin + skew + n] = vals.to(dtype).to(device).reshape(-1)
    assert backing.data_ptr() % 64 == 0
    p = Placed(backing, None, (margin + skew + torch.arange(n, device=device)).reshape(shape))
    p.ptr = backing.data_ptr() + (margin + skew) * backing.element_size()
    return p


def place_flat_int(logical, dtype, skew=0, device='cuda:0'):
    """`place_flat` for int32 / int64 buffers: logical, an integer array of any shape, -> a contiguous INPUT buffer with
    INT_POISON in front of and behind it; that shape as a tuple -> an OUTPUT buffer, the whole allocation full of the
    integer sentinel.  `outside_intact` / `unwritten` work as for the float buffers; `margins_hold(INT_POISON)` checks an
    input the call also writes."""
    assert dtype in (torch.int32, torch.int64)
    is_output = isinstance(logical, tuple)
    shape = logical if is_output else np.shape(logical)
    n = int(np.prod(shape, dtype=np.int64))
    margin = 64 * (1 + skew // 64) + 64
    backing = torch.full((margin + skew + n + 64,), SENTINEL[dtype] if is_output else INT_POISON, dtype=dtype, device=device)
    if not is_output:
        backing[margin + skew:margin + skew + n] = torch.from_numpy(np.ascontiguousarray(logical)).to(dtype).to(device).reshape(-1)
    assert backing.data_ptr() % 64 == 0
    p = Placed(backing, None, (margin + skew + torch.arange(n, device=device)).reshape(shape))
    p.ptr = backing.data_ptr() + (margin + skew) * backing.element_size()
    return p


def read(backing, index):
    """The logical array (float64 numpy) behind a gather index."""
    return backing[index.reshape(-1)].reshape(index.shape).double().cpu().numpy()
