"""A caller-owned workspace of EXACTLY the size a *_workspace_bytes query reports, between two sentinel margins (tests/test_gpu_workspace_bounds.py,
tests/test_workspace_bounds_host.py).  No pytest in here; works on device="cpu" as well (the helper's own test runs there).

Guarded(nbytes, fill, device) is one uint8 allocation [front margin | interior of exactly nbytes | back margin].  The interior is 256-byte aligned (check_workspace asks
for 256 in pq_qlinear_s8_kslabs and pq_qlinear_dyn, for 16 elsewhere) and pre-filled with `fill`; the margins hold a position-dependent byte pattern.  A store that leaves the
interior lands in a margin, inside this allocation, and assert_margins() names it.

patched_allocators(monkeypatch) swaps every workspace allocator of the Python layer for one that hands out the interior of a fresh Guarded of exactly the requested size
(no growth rule, no reuse) and records it; the caller asserts the recorded margins."""
import torch

# Each margin: two of the fused split-K's 256 KiB hand-over slabs (256 x 256 int32 partial sums of one tile: the largest unit any of the workspace-taking kernels writes
# at once — fsk_tail_asm / fsk_sym2_asm / fsk_sym4_asm dump one slab per workgroup) + 4 KiB, so that a hand-over that goes one whole slab too far, or before the first
# one, and still runs over by a row, stays inside this allocation on either side.
SLAB_BYTES = 256 * 256 * 4
MARGIN = 2 * SLAB_BYTES + 4096
ALIGN = 256
GARBAGE = 0xCD                      # what patched_allocators pre-fills with: a workspace "need not be initialised"

_pattern_cache = {}


def _pattern(device, n):
    """n sentinel bytes on `device`: byte i is (167 i + 13) mod 251 — period 251, never constant over two neighbours, so no single fill byte reproduces it"""
    key = (str(device), n)
    if key not in _pattern_cache:
        i = torch.arange(n, dtype=torch.int64, device=device)
        _pattern_cache[key] = ((i * 167 + 13) % 251).to(torch.uint8)
    return _pattern_cache[key]


class Guarded:
    def __init__(self, nbytes, fill=0, device="cuda"):
        assert nbytes >= 0 and 0 <= fill <= 255
        self.nbytes, self.device = int(nbytes), torch.device(device)
        self.buf = torch.empty((MARGIN + ALIGN + self.nbytes + MARGIN,), dtype=torch.uint8, device=self.device)
        self.front = MARGIN + (-(self.buf.data_ptr() + MARGIN)) % ALIGN            # bytes before the interior: MARGIN .. MARGIN + 255
        self.back = self.buf.numel() - self.front - self.nbytes                   # bytes behind it: MARGIN + 1 .. MARGIN + 256
        assert self.front >= MARGIN and self.back >= MARGIN
        self.buf[:self.front] = _pattern(self.device, self.front)
        self.buf[self.front + self.nbytes:] = _pattern(self.device, self.back)
        self.interior = self.buf[self.front:self.front + self.nbytes]
        self.interior.fill_(fill)
        self.ptr = self.buf.data_ptr() + self.front
        assert self.ptr % ALIGN == 0 and self.interior.numel() == self.nbytes

    def refill(self, fill):
        self.interior.fill_(fill)
        return self

    def refill_from(self, other):
        """the interior := the bytes another launch left in ITS interior, repeated to this length (old tickets, ready words and slabs wherever the new launch looks)"""
        assert other.nbytes > 0
        if self.nbytes:
            src = other.interior.to(self.device)
            self.interior.copy_(src.repeat(-(-self.nbytes // other.nbytes))[:self.nbytes])
        return self

    def _margins(self):
        return torch.cat((self.buf[:self.front], self.buf[self.front + self.nbytes:]))

    def _want(self):
        key = (str(self.device), self.front, self.back)
        if key not in _pattern_cache:
            _pattern_cache[key] = torch.cat((_pattern(self.device, self.front), _pattern(self.device, self.back)))
        return _pattern_cache[key]

    def margins_intact(self):
        """a 0-dim bool tensor on the device (no synchronisation): both margins, compared as a whole in one reduction"""
        return (self._margins() == self._want()).all()

    def touched(self):
        """{} or {"front" / "back": (first, last)}: the touched bytes of each margin as offsets from the interior's END (back: 0 = the first byte behind the interior;
        front: -nbytes - 1 = the last byte before its start)"""
        bad = (self._margins() != self._want()).cpu().nonzero().flatten()
        out = {}
        f = bad[bad < self.front]
        b = bad[bad >= self.front] - self.front
        if f.numel():
            out["front"] = (int(f[0]) - self.front - self.nbytes, int(f[-1]) - self.front - self.nbytes)
        if b.numel():
            out["back"] = (int(b[0]), int(b[-1]))
        return out

    def assert_margins(self, what=""):
        if not bool(self.margins_intact()):
            raise AssertionError(self.describe(what))

    def describe(self, what=""):
        """the message of assert_margins for the margins as they are now"""
        msg = []
        for side, (first, last) in self.touched().items():
            at = f"{first} .. {last} from the interior's end" if side == "back" else \
                f"{first} .. {last} from the interior's end (= {first + self.nbytes} .. {last + self.nbytes} from its start)"
            msg.append(f"{side} margin written at bytes {at}")
        return f"{what}: a workspace of {self.nbytes} bytes was overrun: " + ("; ".join(msg) or "a margin was written and has its sentinel again")


def patched_allocators(monkeypatch, fill=GARBAGE):
    """Replace protoquant_amd.qlinear._workspace, the name moe.py bound to it at import, RcclColumnGather._workspace and RcclRowReduceScatter._workspace by allocators
    that return the interior of a fresh Guarded of exactly the requested size.  Returns the list every Guarded handed out is appended to (it also keeps them alive until
    the side stream of an overlapped exchange is through with them)."""
    import importlib
    qlinear = importlib.import_module("protoquant_amd.qlinear")      # (the package attribute of that name is the qlinear CLASS)
    moe, sharded = importlib.import_module("protoquant_amd.moe"), importlib.import_module("protoquant_amd.sharded")
    handed = []

    def exact(device, nbytes):
        g = Guarded(nbytes, fill, device)
        handed.append(g)
        return g.interior

    def gather_ws(self, M, n_total, code, device):
        return exact(device, self._R.lib().pq_allgather_cols_v_workspace_bytes(self.world, M, n_total, code))

    def reduce_ws(self, need, device):
        return exact(device, need)

    monkeypatch.setattr(qlinear, "_workspace", exact)
    monkeypatch.setattr(moe, "_workspace", exact)
    monkeypatch.setattr(sharded.RcclColumnGather, "_workspace", gather_ws)
    monkeypatch.setattr(sharded.RcclRowReduceScatter, "_workspace", reduce_ws)
    return handed
