"""A sentinel arena with guard bands for the buffers of one library call (a helper, not a test; docs/GUARD_BANDS.md).

dkt_amd.ops and dkt_amd.image_data create every output and workspace through `torch.empty` / `empty_like` / `zeros` / `zeros_like` / `ones` / `full`.  A stand-in
for the `torch` module, installed as the `torch` attribute of those modules for the length of a `with` block, serves these six from ONE int32 tensor filled with a
known word, every block aligned to 512 bytes as the caching allocator aligns it and followed by a guard of 64 KiB of fill; `check` runs a call once with the
ordinary allocator and once in a fresh arena per fill word and returns four verdicts:

  footprint     every arena word outside the allocated blocks still holds the fill (head, tail, guards, the slack up to 512 bytes behind a block, the byte behind
                an exact-size workspace), and every input block is bitwise what was put there
  coverage      no element of a returned tensor holds the fill word in BOTH arena runs (an element that was never written)
  independence  every returned tensor is bitwise the same in the two arena runs and in the ordinary run (a result that depends on memory outside its operands
                differs between a NaN fill and a finite one; an accumulation into uninitialised memory too)
  placement     which returned tensors lie inside the arena (the outputs of library calls) and which outside (what torch computed itself), and that a block of
                exactly the size of every non-zero workspace query was taken

What it cannot see: a read past an operand whose value is then masked, a stray write that lands inside another allocated block which is overwritten afterwards,
and a stray write further than the guard behind its block unless it hits an input (footprint) or a returned tensor (independence)."""
import contextlib

import torch

FILL_NAN = 0x7FC07FC0            # a NaN as float32, as two bfloat16 and as two float16; not the 0x7fc00000 the kernels write to poison a failed problem
FILL_FINITE = 0x4B4B4B4B         # 13323083.0 as float32
FILLS = (FILL_NAN, FILL_FINITE)
ALIGN = 512                      # the caching allocator's granularity
GUARD = 64 << 10                 # at least this much fill behind every block
EDGE = 1 << 20                   # fill before the first block and after the last
CHUNK = 32 << 20                 # inputs are compared with what was put there in pieces of this many bytes
BIG = 64 << 20                   # an arena beyond this size has the caching allocator's free blocks released before it is made

_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = size[0]
    return tuple(int(s) for s in size)


def _round_up(n, to):
    return (n + to - 1) // to * to


def _element_size(dtype):
    return torch.empty(0, dtype=dtype).element_size()


class Block:
    def __init__(self, offset, nbytes, dtype, shape, role, address):
        self.offset, self.nbytes, self.dtype, self.shape, self.role, self.address = offset, nbytes, dtype, shape, role, address

    def __repr__(self):
        return "%s block %s %s at +%d (%d bytes)" % (self.role, tuple(self.shape), str(self.dtype).replace("torch.", ""), self.offset, self.nbytes)


class Arena:
    """One int32 tensor filled with `word`; `take` hands out blocks of it (made with `set_` on its storage: plain tensors, not views)."""

    def __init__(self, device, nbytes, word):
        self.device, self.word = torch.device(device), int(word)
        self.nbytes = _round_up(int(nbytes), ALIGN)
        self.buf = torch.full((self.nbytes // 4,), self.word, dtype=torch.int32, device=self.device)
        base = self.buf.data_ptr()
        self.skew = (-base) % ALIGN                     # (allocators align to 512 already; a CPU arena may not be)
        self.cursor = self.skew + EDGE
        self.blocks, self.originals = [], []

    @staticmethod
    def bytes_for(requests):
        """The arena size that holds blocks of these byte counts."""
        return 2 * EDGE + 2 * ALIGN + sum(_round_up(max(int(n), 1), ALIGN) + GUARD for n in requests)

    def take(self, shape, dtype, role="allocated"):
        shape = tuple(int(s) for s in shape)
        t = torch.empty(0, dtype=dtype, device=self.device)
        nbytes = _numel(shape) * t.element_size()
        if self.cursor + _round_up(max(nbytes, 1), ALIGN) + GUARD + EDGE > self.nbytes + self.skew:
            raise RuntimeError("guard arena of %d bytes is full (%d blocks): the measuring run asked for less than this one" % (self.nbytes, len(self.blocks)))
        t.set_(self.buf.untyped_storage(), self.cursor // t.element_size(), shape)
        self.blocks.append(Block(self.cursor, nbytes, dtype, shape, role, t.data_ptr()))
        self.cursor += _round_up(max(nbytes, 1), ALIGN) + GUARD
        return t

    def put(self, tensor):
        """Copy a test input into a block of role `input` (requires_grad carried over: a leaf stays a leaf)."""
        src = tensor.detach()
        block = self.take(src.shape, src.dtype, "input")
        block.copy_(src)
        self.originals.append((self.blocks[-1], src if src.device == self.buf.device else src.to(self.device)))      # (the caller's tensor itself: no second copy)
        return block.requires_grad_(tensor.requires_grad)

    def span(self):
        lo = self.buf.data_ptr()
        return lo, lo + self.buf.numel() * 4

    def contains(self, tensor):
        lo, hi = self.span()
        return lo <= tensor.data_ptr() < hi

    def _fill_bytes(self, start, stop):
        """The fill as bytes [start, stop) of the arena would hold it (little endian)."""
        four = [(self.word >> (8 * k)) & 0xFF for k in range(4)]
        return torch.tensor([four[i % 4] for i in range(start, stop)], dtype=torch.uint8, device=self.device)

    def footprint(self):
        """Failures, a list of strings: gaps between the allocated blocks that no longer hold the fill, input blocks that changed."""
        raw = self.buf.view(torch.uint8)
        blocks = sorted(self.blocks, key=lambda b: b.offset)
        gaps, where, prev_end = [], [], 0                  # (first byte, end) of every stretch that must still be fill
        for b in blocks + [None]:
            start = self.nbytes if b is None else b.offset
            gaps.append((prev_end, start))
            where.append(("before " + repr(b)) if prev_end == 0 else ("behind " + repr(prev)))
            if b is not None:
                prev, prev_end = b, b.offset + b.nbytes
        flags = []
        for lo, hi in gaps:
            mid = min(_round_up(lo, 4), hi)
            ok = (self.buf[mid // 4:hi // 4] == self.word).all()
            if mid > lo:
                ok = ok & (raw[lo:mid] == self._fill_bytes(lo, mid)).all()
            flags.append(ok)
        for block, original in self.originals:
            got, want = raw[block.offset:block.offset + block.nbytes], original.contiguous().reshape(-1).view(torch.uint8)
            same = [(got[i:i + CHUNK] == want[i:i + CHUNK]).all() for i in range(0, block.nbytes, CHUNK)]      # (no comparison result the size of the input)
            flags.append(torch.stack(same).all() if same else torch.ones((), dtype=torch.bool, device=self.device))
        flags = torch.stack(flags).cpu().tolist()
        out = []
        for (lo, hi), w, ok in zip(gaps, where, flags):
            if not ok:
                bad = (raw[lo:hi] != self._fill_bytes(lo, lo + 4).repeat((hi - lo + 3) // 4 + 1)[:hi - lo]).nonzero().reshape(-1)
                out.append("fill overwritten %s: %d bytes, the first at %+d from the gap's start (gap of %d bytes)" % (w, bad.numel(), int(bad[0]), hi - lo))
        for (block, _), ok in zip(self.originals, flags[len(gaps):]):
            if not ok:
                out.append("%r was modified" % block)
        return out


class StandIn:
    """What dkt_amd.ops and dkt_amd.image_data see as `torch`: the six creation functions for tensors on the arena's device come out of the arena, every other
    attribute is torch's.  Without an arena it only measures: the same six delegate to torch and the byte count of each request is kept in `requests`."""

    def __init__(self, device, arena=None):
        self.device, self.arena, self.requests = torch.device(device), arena, []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _here(self, device):
        if device is None:
            return False
        device = torch.device(device)
        return device.type == self.device.type and (device.index is None or self.device.index is None or device.index == self.device.index)

    def _take(self, shape, dtype, kw=None, like=None):
        if kw:                                           # (memory_format, requires_grad, layout ...: a block would not be the tensor torch makes)
            raise TypeError("guard arena: creation keyword(s) %s are not served from the arena; teach tests/guard_arena.py first" % sorted(kw))
        if like is not None and not like.is_contiguous():
            raise TypeError("guard arena: *_like of a non-contiguous tensor %s / %s keeps its strides in torch and would not here" % (tuple(like.shape), like.stride()))
        dtype = dtype or torch.get_default_dtype()
        if self.arena is None:
            self.requests.append(_numel(shape) * _element_size(dtype))
            return torch.empty(shape, dtype=dtype, device=self.device)
        return self.arena.take(shape, dtype)

    def place(self, tensor, dtype=None):
        """A test input on the device: in the arena (role `input`), or where torch puts it when measuring."""
        tensor = tensor.detach().to(dtype or tensor.dtype).requires_grad_(tensor.requires_grad)
        if self.arena is None:
            self.requests.append(tensor.numel() * tensor.element_size())
            return tensor.detach().to(self.device, copy=True).requires_grad_(tensor.requires_grad)
        return self.arena.put(tensor)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._here(device) or kw.get("pin_memory"):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._take(_shape_of(size), dtype, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._here(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._take(_shape_of(size), dtype, kw).fill_(0)

    def ones(self, *size, dtype=None, device=None, **kw):
        if not self._here(device):
            return torch.ones(*size, dtype=dtype, device=device, **kw)
        return self._take(_shape_of(size), dtype, kw).fill_(1)

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._here(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = torch.get_default_dtype() if isinstance(fill_value, float) else torch.int64 if isinstance(fill_value, int) else torch.bool
        return self._take(_shape_of((size,)), dtype, kw).fill_(fill_value)

    def empty_like(self, t, dtype=None, device=None, **kw):
        if not self._here(device or t.device):
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._take(tuple(t.shape), dtype or t.dtype, kw, t)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        if not self._here(device or t.device):
            return torch.zeros_like(t, dtype=dtype, device=device, **kw)
        return self._take(tuple(t.shape), dtype or t.dtype, kw, t).fill_(0)


@contextlib.contextmanager
def installed(monkeypatch, standin, modules):
    """`standin` as the `torch` attribute of `modules` inside the block, the real module again behind it."""
    with monkeypatch.context() as m:
        for mod in modules:
            m.setattr(mod, "torch", standin)
        yield standin


def leaves(value, path="out"):
    """(name, tensor) of every tensor in a return value: tuples, lists and dicts walked, None skipped."""
    if value is None:
        return []
    if isinstance(value, torch.Tensor):
        return [(path, value.detach())]
    if isinstance(value, dict):
        return [x for k, v in value.items() for x in leaves(v, "%s.%s" % (path, k))]
    if isinstance(value, (tuple, list)):
        return [x for i, v in enumerate(value) for x in leaves(v, "%s[%d]" % (path, i))]
    return []


def _bits(t):
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.view(_INT_OF_SIZE[t.element_size()])


def _fill_mask(t, word):
    """Which elements of t hold the fill bit for bit."""
    size = t.element_size()
    if size == 1:                                        # the fill's bytes alternate: by address
        t = t.contiguous()
        four = torch.tensor([(word >> (8 * k)) & 0xFF for k in range(4)], dtype=torch.uint8, device=t.device)
        at = (torch.arange(t.numel(), device=t.device) + t.data_ptr() % 4) % 4
        return (_bits(t).reshape(-1) == four[at]).reshape(t.shape)
    pattern = {2: word & 0xFFFF, 4: word, 8: word | (word << 32)}[size]
    return _bits(t) == pattern


def _same(a, b, tol):
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape / dtype %s %s vs %s %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    if a.numel() == 0:
        return None
    differ = _bits(a) != _bits(b)
    n = int(differ.sum())
    if n == 0:
        return None
    if tol is not None and a.dtype.is_floating_point and torch.allclose(a.double(), b.double(), rtol=tol[0], atol=tol[1], equal_nan=True):
        return None
    d = (a.double() - b.double())[differ]
    finite = d[torch.isfinite(d)].abs()
    return "%d of %d elements differ (max |d| %s, %d not finite on one side)" % (n, a.numel(), "%.3g" % float(finite.max()) if finite.numel() else "-",
                                                                                 d.numel() - finite.numel())


class Report:
    """The verdicts of one `check`: lists of failure strings (empty = passed), and what the arena runs recorded."""

    def __init__(self):
        self.footprint, self.coverage, self.independence, self.placement = [], [], [], []
        self.inside, self.blocks, self.queries, self.results = {}, [], [], None

    def outside(self):
        return sorted(k for k, v in self.inside.items() if not v)

    def failures(self, outside=(), exempt=()):
        """Every failed verdict as one list.  `outside`: the returned tensors the case says torch computed itself; `exempt`: returned tensors whose content a
        header leaves unspecified (coverage only)."""
        out = ["footprint: " + f for f in self.footprint]
        out += ["coverage: " + f for name, f in self.coverage if name not in exempt]
        out += ["independence: " + f for f in self.independence]
        out += ["placement: " + f for f in self.placement]
        if sorted(outside) != self.outside():
            out.append("placement: outside the arena %s, the case says %s" % (self.outside(), sorted(outside)))
        return out


def check(call, inputs, device, monkeypatch, modules, extra=None, tol=None, sync=None):
    """Run `call(placed inputs)` with the ordinary allocator, then in a fresh arena per fill word, and compare (the module's docstring).
    inputs: name -> tensor, put into the arena before the call; extra(standin, report): a context manager around every run (further patches and recorders of the
    case; standin.arena is None in the ordinary run); tol = (rtol, atol): independence of a call that is not deterministic by itself."""
    device = torch.device(device)
    sync = sync or (torch.cuda.synchronize if device.type == "cuda" else (lambda: None))
    extra = extra or (lambda standin, report: contextlib.nullcontext())
    report = Report()

    def one(standin):
        with installed(monkeypatch, standin, modules), extra(standin, report):
            placed = {k: standin.place(v) for k, v in inputs.items()}
            value = call(placed)
            sync()
        return leaves(value)

    measure = StandIn(device)
    plain = one(measure)                                  # builds and loads the libraries, fills the caches outside the arena, sizes the arena
    runs = []
    for word in FILLS:
        nbytes = Arena.bytes_for(measure.requests)
        if device.type == "cuda" and nbytes > BIG:        # (what the ordinary run and the last arena freed goes back to the device first)
            torch.cuda.empty_cache()
        arena = Arena(device, nbytes, word)
        report.queries = []
        got = one(StandIn(device, arena))
        report.footprint += ["fill %#x: %s" % (word, f) for f in arena.footprint()]
        inside = {name: arena.contains(t) for name, t in got if t.numel()}
        if report.inside and inside != report.inside:
            report.placement.append("the two arena runs place their results differently: %s vs %s" % (report.inside, inside))
        report.inside = inside
        report.blocks = list(arena.blocks)
        taken = [b.nbytes for b in arena.blocks if b.role == "allocated"]
        for name, nbytes in report.queries:
            if nbytes and _round_up(nbytes, 4) not in taken:
                report.placement.append("%s asked for %d bytes and no block of that size was taken (blocks: %s)" % (name, nbytes, sorted(set(taken))))
        runs.append([(name, t.clone(), _fill_mask(t, word)) for name, t in got])       # (out of the arena before it is freed)
        del arena, got
    a, b = runs
    if [n for n, _ in plain] != [n for n, _, _ in a] or [n for n, _, _ in a] != [n for n, _, _ in b]:
        report.independence.append("the runs return different structures")
        return report
    for (name, t0), (_, ta, ma), (_, tb, mb) in zip(plain, a, b):
        unwritten = int((ma & mb).sum()) if ta.numel() else 0
        if unwritten:
            first = (ma & mb).reshape(-1).nonzero()[0]
            report.coverage.append((name, "%s %s: %d of %d elements never written, the first at flat index %d" % (name, tuple(ta.shape), unwritten, ta.numel(),
                                                                                                               int(first))))
        if unwritten:                                     # (reported once, by coverage: the comparison below is about the elements that were written)
            t0, ta, tb = (torch.where(ma & mb, torch.zeros((), dtype=x.dtype, device=x.device), x) for x in (t0, ta, tb))
        for what, x, y in (("NaN fill vs finite fill", ta, tb), ("ordinary allocator vs arena", t0, ta)):
            diff = _same(x, y, tol)
            if diff:
                report.independence.append("%s %s, %s: %s" % (name, tuple(ta.shape), what, diff))
    report.results = dict(plain)
    return report
