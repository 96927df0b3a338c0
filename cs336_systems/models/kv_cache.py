"""Key / value cache of ``BasicsTransformerLM.forward_cached``.

``k`` and ``v`` are ``(L, B, H, max_len, d)``: ``cache.k[l]`` is the ``(B, H, max_len, d)`` view the
decode-attention kernel reads in place (layer and batch are the outer dims, so a layer slice or a
batch sub-view needs no copy). K rows are stored rotated (RoPE at the row's position). ``lengths``
is the per-sequence int32 length on the device (what the kernels read); ``length`` is its host
mirror: ``generate`` batches are rectangular, so one number describes them all and no step has to
read the device tensor back.

``fp8=True``: ``k`` and ``v`` are ``torch.float8_e4m3fn`` planes of the same shape and ``k_scale`` /
``v_scale`` ``(L, B, H, max_len)`` fp32 planes hold one scale per cached row, the row being
``bytes * scale[row]`` (``ops/decode.py``): ``d + 4`` bytes per row instead of ``2 d``. Rows are
quantized when they are written and never again. ``dtype`` stays the compute dtype (what q and the
attention output are).

:class:`PagedKVCache` stores the same rows in fixed-size pages of one pool behind a block table,
allocated as the sequences grow and shareable between sequences; see its docstring."""

from __future__ import annotations

import torch


class KVCache:
    def __init__(self, model_or_dims, batch: int, max_len: int | None = None, device=None, dtype=None,
                 fp8: bool = False):
        """``model_or_dims``: a ``BasicsTransformerLM`` (layers, heads, head dim, ``context_length``,
        device and parameter dtype are taken from it) or ``(num_layers, num_heads, d_head)``."""
        if isinstance(model_or_dims, (tuple, list)):
            L, H, d = (int(x) for x in model_or_dims)
            if max_len is None:
                raise ValueError("KVCache from dims needs max_len")
        else:
            m = model_or_dims
            attn = m.layers[0].attn
            L, H, d = len(m.layers), attn.num_heads, attn.d_k
            w = attn.q_proj.weight
            if max_len is None:
                max_len = m.context_length
            if device is None:
                device = w.device
            if dtype is None:
                dtype = w.dtype
        if batch < 1 or max_len < 1:
            raise ValueError("KVCache needs batch >= 1 and max_len >= 1")
        self.num_layers, self.batch, self.num_heads, self.max_len, self.d_head = L, int(batch), H, int(max_len), d
        self.fp8 = bool(fp8)
        self._dtype = torch.empty((), dtype=dtype).dtype  # (None: the default dtype, as torch.zeros takes it)
        if self.fp8:
            self.k = torch.zeros(L, batch, H, max_len, d, device=device, dtype=torch.uint8).view(torch.float8_e4m3fn)
            self.v = torch.zeros_like(self.k)
            self.k_scale = torch.ones(L, batch, H, max_len, device=device, dtype=torch.float32)
            self.v_scale = torch.ones_like(self.k_scale)
        else:
            self.k = torch.zeros(L, batch, H, max_len, d, device=device, dtype=dtype)
            self.v = torch.zeros_like(self.k)
            self.k_scale = self.v_scale = None
        self.lengths = torch.zeros(batch, dtype=torch.int32, device=device)
        self.length = 0

    @property
    def device(self):
        return self.k.device

    @property
    def dtype(self):
        """The compute dtype: the planes' own for a plain cache, the one given for an FP8 cache."""
        return self._dtype

    @property
    def nbytes(self) -> int:
        """Bytes of the K / V planes (and their scale planes)."""
        return sum(t.numel() * t.element_size() for t in (self.k, self.v, self.k_scale, self.v_scale) if t is not None)

    def reset(self) -> None:
        """Forget every cached token (the rows are not cleared: rows beyond ``length`` are never read)."""
        self.lengths.zero_()
        self.length = 0

    def truncate(self, length: int) -> None:
        """Forget the tokens at and beyond ``length`` (rejected draft tokens of a speculative round;
        their rows stay and are overwritten). In place and without a host sync, so a ``DecodeGraph``
        tied to this cache stays valid."""
        length = int(length)
        if length < 0 or length > self.length:
            raise ValueError(f"truncate({length}) on a cache of length {self.length}")
        self.lengths.fill_(length)
        self.length = length

    def advance(self, n: int) -> None:
        self.lengths += n
        self.length += n

    def __repr__(self):
        return (f"KVCache(layers={self.num_layers}, batch={self.batch}, heads={self.num_heads}, "
                f"max_len={self.max_len}, d_head={self.d_head}, length={self.length}, dtype={self.dtype}"
                f"{', format=e4m3 rows + fp32 row scales' if self.fp8 else ''})")


PAGE_SIZES = (16, 32, 64, 128, 256)


class _PagePool:
    """What a :class:`PagedKVCache` and its ``row`` views share: the planes, the whole table and the
    host-side allocator (free list, per-page reference counts, per-sequence page lists and lengths)."""

    def __init__(self, k, v, block_table, lengths):
        self.k, self.v, self.block_table, self.lengths = k, v, block_table, lengths
        num_pages = k.shape[1]
        self.free = list(range(num_pages - 1, -1, -1))  # a stack: pages are handed out from id 0 up
        self.refs = [0] * num_pages
        self.pages = [[] for _ in range(block_table.shape[0])]  # sequence -> its page ids, in order
        self.len = [0] * block_table.shape[0]

    # every device update is a fill of a view with a host scalar: a launch, never a read-back, and the
    # value is baked into the launch (no staging buffer that a later host write could race with)
    def set_entry(self, s: int, i: int, page: int) -> None:
        self.block_table[s, i:i + 1].fill_(page)

    def take(self) -> int:
        page = self.free.pop()
        self.refs[page] = 1
        return page

    def drop(self, page: int) -> None:
        self.refs[page] -= 1
        if self.refs[page] == 0:
            self.free.append(page)

    def released_by(self, pages) -> int:
        """How many pages return to the free list when the references ``pages`` (ids, with repeats) go."""
        count = {}
        for p in pages:
            count[p] = count.get(p, 0) + 1
        return sum(1 for p, c in count.items() if self.refs[p] == c)

    def copy_page(self, src: int, dst: int) -> None:
        self.k[:, dst].copy_(self.k[:, src])  # device to device, all layers
        self.v[:, dst].copy_(self.v[:, src])


class PagedKVCache:
    """A KV cache whose rows live in fixed-size pages of one pool, addressed through a block table.

    ``k`` / ``v`` are ``(L, num_pages, H, page_size, d)``: ``cache.k[l]`` is the ``(num_pages, H,
    page_size, d)`` view the paged kernels read in place (``csrc/flash_attn/fa_decode_paged.hip``); one
    page id means the same page index in every layer. Row ``j`` of sequence ``b`` is row ``j % page_size``
    of page ``block_table[b, j // page_size]``. ``block_table`` ``(B, ceil(max_len / page_size))`` int32
    and ``lengths`` ``(B,)`` int32 live on the device at fixed addresses (a ``DecodeGraph`` captures
    them); a table entry that holds no page is ``-1``. K rows are stored rotated.

    The allocator is host-side Python -- a free list and per-page reference counts -- and never reads
    the device: the host mirrors lengths and table, and every table / length update is a device-side
    fill issued from the host without synchronisation. ``num_pages=None`` is ``batch * ceil(max_len /
    page_size)``, which cannot run out; a smaller pool is the point. Rules:

    * ``reserve(n)`` gives every sequence pages for slots ``[length_b, length_b + n)`` or raises
      ``RuntimeError("out of pages ...")`` before changing anything;
    * ``fork(src, dst)`` shares ``src``'s full pages by reference count and copies its last, partially
      filled page, so full shared pages are never written: appends go to slots at or beyond the length,
      which are always in a private page;
    * ``truncate`` into a shared page gives the sequence a private copy of it;
    * ``reset`` / ``truncate`` / ``free`` return the pages whose count drops to 0.

    Sequences may have different lengths at this level (``seq_lengths``); ``length`` is the common one
    and raises ``ValueError`` when they differ (``forward_cached`` and ``generate`` are rectangular)."""

    def __init__(self, model_or_dims, batch: int, page_size: int = 64, num_pages: int | None = None,
                 max_len: int | None = None, device=None, dtype=None, fp8: bool = False):
        if fp8:
            raise NotImplementedError("PagedKVCache has no FP8 format (out of scope)")
        if isinstance(model_or_dims, (tuple, list)):
            L, H, d = (int(x) for x in model_or_dims)
            if max_len is None:
                raise ValueError("PagedKVCache from dims needs max_len")
        else:
            m = model_or_dims
            attn = m.layers[0].attn
            L, H, d = len(m.layers), attn.num_heads, attn.d_k
            w = attn.q_proj.weight
            if max_len is None:
                max_len = m.context_length
            if device is None:
                device = w.device
            if dtype is None:
                dtype = w.dtype
        if page_size not in PAGE_SIZES:
            raise ValueError(f"PagedKVCache page_size must be one of {PAGE_SIZES} (got {page_size})")
        if batch < 1 or max_len < 1:
            raise ValueError("PagedKVCache needs batch >= 1 and max_len >= 1")
        per_seq = -(-int(max_len) // page_size)
        if num_pages is None:
            num_pages = batch * per_seq
        if num_pages < 1:
            raise ValueError("PagedKVCache needs num_pages >= 1")
        self.num_layers, self.batch, self.num_heads, self.max_len, self.d_head = L, int(batch), H, int(max_len), d
        self.page_size, self.num_pages, self.pages_per_sequence = int(page_size), int(num_pages), per_seq
        self.fp8 = False
        self.k_scale = self.v_scale = None
        k = torch.zeros(L, num_pages, H, page_size, d, device=device, dtype=dtype)
        self._pool = _PagePool(k, torch.zeros_like(k),
                               torch.full((batch, per_seq), -1, dtype=torch.int32, device=k.device),
                               torch.zeros(batch, dtype=torch.int32, device=k.device))
        self._seqs = list(range(batch))
        self._bind()

    def _bind(self) -> None:
        pool, s = self._pool, self._seqs
        self.k, self.v = pool.k, pool.v
        whole = len(s) == pool.block_table.shape[0]
        self.block_table = pool.block_table if whole else pool.block_table[s[0]:s[0] + 1]
        self.lengths = pool.lengths if whole else pool.lengths[s[0]:s[0] + 1]

    def row(self, b: int) -> "PagedKVCache":
        """Sequence ``b`` as a batch-1 cache on the same pool, allocator, table row and length (views):
        the prefill of a shared prompt runs through it."""
        if not 0 <= b < self.batch:
            raise IndexError(f"row({b}) of a cache with batch {self.batch}")
        r = object.__new__(PagedKVCache)
        r.__dict__.update(self.__dict__)
        r.batch, r._seqs = 1, [self._seqs[b]]
        r._bind()
        return r

    @property
    def device(self):
        return self.k.device

    @property
    def dtype(self):
        return self.k.dtype

    @property
    def nbytes(self) -> int:
        """Bytes of the pool's K / V planes and the table."""
        return sum(t.numel() * t.element_size() for t in (self.k, self.v, self._pool.block_table))

    @property
    def pages_free(self) -> int:
        return len(self._pool.free)

    @property
    def pages_in_use(self) -> int:
        return self.num_pages - len(self._pool.free)

    @property
    def seq_lengths(self) -> list:
        """The host mirror of ``lengths``."""
        return [self._pool.len[s] for s in self._seqs]

    @property
    def length(self) -> int:
        ls = self.seq_lengths
        if any(x != ls[0] for x in ls):
            raise ValueError(f"PagedKVCache.length: the sequences differ ({ls}); see seq_lengths")
        return ls[0]

    @length.setter
    def length(self, value: int) -> None:
        # The host mirror alone (a DecodeGraph after a replay, whose captured ``lengths += n`` advanced
        # the device tensor, and around its warm-up); everything else goes through the methods below.
        for s in self._seqs:
            self._pool.len[s] = int(value)

    def reserve(self, n: int = 1) -> None:
        """Make sure every sequence owns pages for slots ``[length_b, length_b + n)``."""
        pool, P = self._pool, self.page_size
        need = []
        for s in self._seqs:
            if pool.len[s] + n > self.pages_per_sequence * P:
                raise ValueError(f"{pool.len[s]} cached + {n} new tokens exceed the table "
                                 f"({self.pages_per_sequence} pages of {P})")
            need.append(max(0, -(-(pool.len[s] + n) // P) - len(pool.pages[s])) if n > 0 else 0)
        if sum(need) > len(pool.free):
            raise RuntimeError(f"out of pages: {sum(need)} needed, {len(pool.free)} of {self.num_pages} free")
        for s, m in zip(self._seqs, need):
            for _ in range(m):
                page = pool.take()
                pool.set_entry(s, len(pool.pages[s]), page)
                pool.pages[s].append(page)

    def advance(self, n: int) -> None:
        self.lengths += n
        for s in self._seqs:
            self._pool.len[s] += n

    def _release_from(self, s: int, keep: int) -> None:
        """Give back sequence ``s``'s pages from index ``keep`` on."""
        pool = self._pool
        while len(pool.pages[s]) > keep:
            pool.drop(pool.pages[s].pop())
            pool.set_entry(s, len(pool.pages[s]), -1)

    def free(self, b: int) -> None:
        """Release sequence ``b``: its pages go back (those no one else holds) and its length is 0."""
        s = self._seqs[b]
        self._release_from(s, 0)
        self._pool.len[s] = 0
        self._pool.lengths[s:s + 1].zero_()

    def reset(self) -> None:
        """Forget every cached token and return every page."""
        for b in range(self.batch):
            self.free(b)

    def truncate(self, length: int) -> None:
        """Forget the tokens at and beyond ``length`` (of every sequence): pages wholly beyond it go
        back, and if slot ``length`` falls into a page that another sequence shares, the sequence gets
        a private copy of that page, so that no later append lands in a shared one. No host sync."""
        pool, P = self._pool, self.page_size
        length = int(length)
        if length < 0 or any(length > pool.len[s] for s in self._seqs):
            raise ValueError(f"truncate({length}) on a cache of lengths {self.seq_lengths}")
        keep = -(-length // P)
        partial = length % P != 0
        private = [s for s in self._seqs if partial and pool.refs[pool.pages[s][keep - 1]] > 1]
        gone = [p for s in self._seqs for p in pool.pages[s][keep:]]
        if len(private) > len(pool.free) + pool.released_by(gone):
            raise RuntimeError(f"out of pages: {len(private)} needed to privatise shared pages, "
                               f"{len(pool.free)} of {self.num_pages} free")
        for s in self._seqs:
            self._release_from(s, keep)
            pool.len[s] = length
        for s in private:
            old = pool.pages[s][keep - 1]
            if pool.refs[old] == 1:  # the other holders were truncated away just now
                continue
            new = pool.take()
            pool.copy_page(old, new)
            pool.drop(old)
            pool.pages[s][keep - 1] = new
            pool.set_entry(s, keep - 1, new)
        self.lengths.fill_(length)

    def fork(self, src: int, dst=None) -> None:
        """Make every sequence in ``dst`` (default: all others) a continuation of ``src``: it is freed,
        then shares ``src``'s full pages, gets a fresh copy of ``src``'s last, partially filled page
        (device to device, all layers) and takes ``src``'s length."""
        pool, P = self._pool, self.page_size
        if dst is None:
            dst = [b for b in range(self.batch) if b != src]
        dst = [int(b) for b in ([dst] if isinstance(dst, int) else dst)]
        if not 0 <= src < self.batch or any(not 0 <= b < self.batch or b == src for b in dst) \
                or len(set(dst)) != len(dst):
            raise ValueError(f"fork({src}, {dst}) on a cache with batch {self.batch}")
        s0 = self._seqs[src]
        n = pool.len[s0]
        full, tail = n // P, n % P != 0
        gone = [p for b in dst for p in pool.pages[self._seqs[b]]]
        if tail and len(dst) > len(pool.free) + pool.released_by(gone):
            raise RuntimeError(f"out of pages: {len(dst)} needed for the copies of the last page, "
                               f"{len(pool.free)} of {self.num_pages} free")
        for b in dst:
            self.free(b)
        for b in dst:
            s = self._seqs[b]
            for i in range(full):
                page = pool.pages[s0][i]
                pool.refs[page] += 1
                pool.pages[s].append(page)
                pool.set_entry(s, i, page)
            if tail:
                page = pool.take()
                pool.copy_page(pool.pages[s0][full], page)
                pool.pages[s].append(page)
                pool.set_entry(s, full, page)
            pool.len[s] = n
            pool.lengths[s:s + 1].fill_(n)

    def gather(self, l: int | None = None):
        """Dense ``(B, H, max_len, d)`` K and V of layer ``l`` (``(L, B, H, max_len, d)`` for ``None``),
        rows at and beyond each sequence's length zeroed. For tests and debugging."""
        from ..ops.decode import paged_gather

        if l is None:
            ks, vs = zip(*(self.gather(i) for i in range(self.num_layers)))
            return torch.stack(ks), torch.stack(vs)
        live = (torch.arange(self.max_len, device=self.k.device)[None, :] < self.lengths.to(torch.int64)[:, None])
        live = live[:, None, :, None]
        out = []
        for plane in (self.k[l], self.v[l]):
            dense = paged_gather(plane, self.block_table)[:, :, :self.max_len]
            out.append(torch.where(live, dense, torch.zeros_like(dense)))
        return out[0], out[1]

    def __repr__(self):
        try:
            length = str(self.length)
        except ValueError:
            length = str(self.seq_lengths)
        return (f"PagedKVCache(layers={self.num_layers}, batch={self.batch}, heads={self.num_heads}, "
                f"max_len={self.max_len}, d_head={self.d_head}, page_size={self.page_size}, "
                f"pages={self.pages_in_use}/{self.num_pages} in use, length={length}, dtype={self.dtype})")
