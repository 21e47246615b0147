"""MetaLM (reference metagym/metalm/metalm.py) with its rows drawn on the GPU by `mg_metalm_generate`."""
import math

import numpy as np

from .. import _lib


def default_element_capacity(n, l):
    """Tokens one row's element table holds: n * ceil(l + 8 sqrt(l) + 8). An element is longer than ceil(l + 8 sqrt(l) + 8)
    with probability below 2e-15 for every l > 1 (Poisson tail, worst near l = 64), so a row overflows this capacity with
    probability below n * 2e-15; when one does, the call raises and names the row, it never truncates."""
    return int(n) * int(math.ceil(l + 8.0 * math.sqrt(l) + 8.0))


class MetaLM(object):
    """MetaLM(V, n, l, e, L): rows of n Poisson(l)-length token elements repeated until length L, each repetition noised
    with probability e per token (and a noised token masked to 0 with probability mask_ratio). Attributes and properties
    are the reference's; `mask_ratio` is settable.

    Every row is bit for bit what the reference draws from numpy's legacy MT19937 stream:
      - `batch_generator(B)` (no seed) continues numpy.random's global stream like the reference's batch_generator, row
        after row, and leaves the global state where the reference leaves it (one wave on the device: serial, the drop-in
        path).
      - `batch_generator(B, seed=s)` / `seeds=[...]` draws row t from its own stream numpy.random.seed(s + t) /
        seeds[t], all rows in parallel (the fast path). This is the one semantic change against the reference: seeded rows
        are independent streams, not one stream across the batch. numpy.random's global state is not touched.
    `element_capacity` bounds the tokens of one row's n elements (default `default_element_capacity(n, l)`); a row that
    needs more raises `MetaGymHipError` naming it. There is no CPU path: device must be a ROCm GPU.
    """

    def __init__(self, V=64, n=10, l=64, e=0.10, L=2048, device="cuda", element_capacity=None):
        self.L = int(L)
        self.V = int(V)
        self.lamb = l
        self.n = n
        self.e = float(e)
        self.mask_ratio = 0.30
        assert n > 1 and V > 1 and l > 1 and e > 0 and e < 1 and L > 1
        import torch
        if torch.device(device).type != "cuda":
            raise _lib.MetaGymHipError("metagym_amd runs on an AMD GPU only (got device %r); there is no CPU fallback"
                                       % (device,))
        self.device = _lib.canonical_device(device)
        self.element_capacity = int(element_capacity) if element_capacity is not None else \
            default_element_capacity(n, l)
        self.last_overflow = None
        _lib.load()

    @property
    def VocabSize(self):
        return self.V + 2

    @property
    def SepID(self):
        return self.V + 1

    @property
    def MaskID(self):
        return 0

    @property
    def PaddingID(self):
        return 0

    def _params(self):
        p = _lib.MetaLMParams()
        p.V, p.n, p.L = self.V, int(self.n), self.L
        p.l, p.e, p.mask_ratio = float(self.lamb), self.e, float(self.mask_ratio)
        return p

    def _out(self, B, out):
        import torch
        if out is None:
            return (torch.empty(B, self.L, dtype=torch.int32, device=self.device),
                    torch.empty(B, self.L, dtype=torch.int32, device=self.device))
        features, labels = out
        for t in (features, labels):
            if t.dtype != torch.int32 or tuple(t.shape) != (B, self.L) or t.device != self.device or not t.is_contiguous():
                raise ValueError("out tensors must be contiguous int32 [%d, %d] on %s" % (B, self.L, self.device))
        return features, labels

    def _raise_overflow(self, row):
        raise _lib.MetaGymHipError(
            "MetaLM row %d needs more than element_capacity = %d element tokens (n = %s, l = %s); pass a larger "
            "element_capacity" % (row, self.element_capacity, self.n, self.lamb))

    def batch_generator(self, batch_size, seed=None, seeds=None, out=None, check=True):
        """`batch_size` rows as int32 device tensors (features, labels), each [batch_size, L].

        seed / seeds: seeded mode, row t from numpy.random.seed(seed + t) or seeds[t] (32-bit values; the same contract
        as MazeTaskManager.sample_tasks_device). Both None: chained mode on numpy.random's global stream.
        out: optional (features, labels) to write into. check=False skips the overflow read after a seeded launch (no
        synchronisation; `self.last_overflow` then holds the device word: INT32_MAX, or the first overflowing row).
        Chained mode always synchronises (it hands the stream back to numpy.random) and always checks."""
        import torch
        lib = _lib.load()
        B = int(batch_size)
        if B <= 0:
            raise ValueError("batch_size must be positive")
        features, labels = self._out(B, out)
        ovf = torch.empty(1, dtype=torch.int32, device=self.device)
        self.last_overflow = ovf
        stream = _lib.current_stream(self.device)
        p = self._params()
        if seed is None and seeds is None:
            st = np.random.get_state()
            if st[0] != "MT19937":
                raise ValueError("numpy.random's global generator is not MT19937")
            state = np.empty(625, np.uint32)
            state[:624] = st[1]
            state[624] = st[2]
            mt = torch.from_numpy(state.view(np.int32)).to(self.device)
            rc = lib.mg_metalm_generate(p, B, 0, None, _lib.ptr(mt), self.element_capacity, _lib.ptr(features),
                                        _lib.ptr(labels), _lib.ptr(ovf), stream)
            _lib.check(rc, "mg_metalm_generate")
            row = int(ovf.item())
            if row < B:
                self._raise_overflow(row)
            state = mt.cpu().numpy().view(np.uint32)
            np.random.set_state((st[0], state[:624].copy(), int(state[624]), st[3], st[4]))
            return features, labels
        seeds_t = None
        if seeds is not None:
            arr = np.asarray(seeds.cpu().numpy() if hasattr(seeds, "cpu") else seeds, dtype=np.int64)
            if arr.shape != (B,) or arr.min() < 0 or arr.max() >= 2 ** 32:
                raise ValueError("seeds must be %d values in [0, 2^32)" % B)
            seeds_t = torch.from_numpy(arr.astype(np.uint32).view(np.int32)).to(self.device)
            seed = 0
        if not (0 <= int(seed) and int(seed) + B <= 2 ** 32):
            raise ValueError("seeds are 32-bit (numpy.random.seed's integer range): need 0 <= seed and seed + B <= 2^32")
        rc = lib.mg_metalm_generate(p, B, int(seed), _lib.ptr(seeds_t), None, self.element_capacity, _lib.ptr(features),
                                    _lib.ptr(labels), _lib.ptr(ovf), stream)
        _lib.check(rc, "mg_metalm_generate")
        if check:
            row = int(ovf.item())
            if row < B:
                self._raise_overflow(row)
        return features, labels

    def data_generator(self, seed=None):
        """One row: (features [L], labels [L]). seed=None continues numpy.random's global stream like the reference."""
        f, lb = self.batch_generator(1, seed=seed)
        return f[0], lb[0]

    def generate_to_file(self, size, output_stream, seed=None):
        """The reference's text format: one line per row, tab-separated "feature,label" pairs. output_stream is a path
        (opened, written, closed) or anything with write()."""
        f, lb = self.batch_generator(size, seed=seed)
        f, lb = f.cpu().numpy(), lb.cpu().numpy()
        need_close = isinstance(output_stream, str)
        if need_close:
            output_stream = open(output_stream, "w")
        try:
            for i in range(f.shape[0]):
                output_stream.write("\t".join("%d,%d" % (a, b) for a, b in zip(f[i].tolist(), lb[i].tolist())))
                output_stream.write("\n")
        finally:
            if need_close:
                output_stream.close()
