"""``CompressedLatents`` -- a compressed dataset that stays compressed and serves minibatches.

The reference reads a ``.bin`` container back in one piece (``decompress_dataset``, hub/compressor.py:209-254: every
record in file order, stacked into a host float32 [N,512] array, 2 KB per image against the ~190 B it takes on disk).
The consumer the representations are compressed FOR -- a downstream predictor trained from the compressed copy --
draws shuffled minibatches and wants them on the device.  This class keeps the container body and its record offsets
resident (in HBM, or in host memory for ``device="cpu"``) and decodes the rows of any index vector with one launch of
``lla_rans_decode_gather`` (gather + rANS decode + dequantise, csrc/entropy.hip; ``lla_rans_decode_gather_host`` on the
host): same values, bit for bit, as ``decompress_dataset(...)[indices]``.

``HyperpriorLatents`` is the same surface over a scale-hyperprior container (two records per image, lossyless/rates.py:
715-724 for the images named): a gather of the side records, ``z_encoder`` on the fp32 GEMM, then a gathered conditional
decode (``lla_rans_decode_gather_strided``, ``lla_gemm_f32``, ``lla_gaussian_decode_gather``), on the GPU only.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .entropy import resident_takes

_DTYPES = {torch.float32: _lib.LLA_Z_F32, torch.float16: _lib.LLA_Z_F16}


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _read_container(file):
    """-> (record count, body uint8 padded by a word, record offsets uint64 [n + 1]) of a container file."""
    blob = np.fromfile(str(file), dtype=np.uint8)
    L = _lib.lib()
    n = ctypes.c_uint32(0)
    # (validates the count against the file size before anything is sized by it)
    _lib.check(L.lla_container_index(_np_ptr(blob), blob.size, None, 0, ctypes.byref(n)), "lla_container_index")
    off = np.zeros(int(n.value) + 1, dtype=np.uint64)
    _lib.check(L.lla_container_index(_np_ptr(blob), blob.size, _np_ptr(off), off.size, ctypes.byref(n)),
               "lla_container_index")
    body = blob[4:]
    # padded as ClipCompressor._decode_records pads it: streams are read as whole 32-bit words
    return int(n.value), np.concatenate([body, np.zeros((-len(body)) % 4 + 4, np.uint8)]), off


class _Latents:
    """What the resident datasets share: index handling, the ``out`` argument, statuses, labels and the minibatch iterator.
    A subclass sets ``device``, ``z_dim``, ``_n``, ``_body``, ``_off``, ``_labels`` and implements
    ``_decode(idx, B, out, ld, dtype) -> status`` (int32 [B] on ``device``: 0 decoded, 1 malformed stream, 2 index out
    of range; such rows zeroed)."""

    def _set_device(self, device, no_gpu):
        self.device = torch.device(device)
        if self.device.type == "cuda" and not torch.cuda.is_available():
            raise RuntimeError(no_gpu)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    def _load_labels(self, label_file):
        self._labels = None
        if label_file is not None:
            y = np.load(label_file, allow_pickle=False).astype(np.int64)
            if y.shape[0] != self._n:
                raise ValueError(f"{label_file} holds {y.shape[0]} labels for {self._n} records")
            self._labels = torch.from_numpy(y).to(self.device)

    def __len__(self):
        return self._n

    @property
    def nbytes(self):
        """Compressed bytes resident: the container body and its record offsets."""
        return int(self._body.nbytes + self._off.nbytes)

    # ------------------------------------------------------------------ indexing
    def _index(self, indices):
        """-> int64 index tensor on ``self.device`` (1-D, contiguous)."""
        if isinstance(indices, torch.Tensor):
            idx = indices
        else:
            idx = torch.from_numpy(np.asarray(indices, dtype=np.int64))
        if idx.dtype != torch.int64:
            if idx.is_floating_point() or idx.dtype == torch.bool:
                raise TypeError("indices must be integers")
            idx = idx.to(torch.int64)
        return idx.reshape(-1).to(self.device).contiguous()

    def take(self, indices, dtype=torch.float32, out=None, check=True):
        """Rows ``indices`` (list, numpy array or integer tensor on any device; repeats allowed) ->
        ``[len(indices), z_dim]`` of ``dtype`` (float32 or float16) on ``self.device``, written into ``out`` if given.

        ``check=True`` reads the per-row status back (one synchronisation): ``IndexError`` for an index outside
        ``[0, N)`` -- negative indices do not wrap around -- and ``ValueError`` for a malformed stream.  With
        ``check=False`` nothing is read back; such rows are all zero."""
        if dtype not in _DTYPES:
            raise TypeError("dtype must be torch.float32 or torch.float16")
        idx = self._index(indices)
        B, C = int(idx.numel()), self.z_dim
        if out is None:
            out = torch.empty((B, C), dtype=dtype, device=self.device)
        elif (out.dtype != dtype or out.device != self.device or out.dim() != 2 or tuple(out.shape) != (B, C)
              or out.stride(1) != 1 or (B > 1 and out.stride(0) < C)):
            raise ValueError(f"out must be a [{B}, {C}] {dtype} tensor on {self.device} with contiguous rows")
        if B == 0:
            return out
        ld = int(out.stride(0)) if B > 1 else C
        status = self._decode(idx, B, out, ld, dtype)
        if check:
            worst = int(status.max())
            if worst == 2:
                bad = int(idx[status == 2][0])
                raise IndexError(f"index {bad} is out of range for {self._n} records (negative indices do not wrap)")
            if worst != 0:
                raise ValueError("malformed rANS stream in container")
        return out

    def __getitem__(self, key):
        if isinstance(key, slice):
            return self.take(torch.arange(*key.indices(self._n)))
        if isinstance(key, (int, np.integer)):
            return self.take([int(key)])[0]
        return self.take(key)

    def labels(self, indices):
        """Labels of rows ``indices`` (int64 on ``self.device``); ``IndexError`` outside ``[0, N)``."""
        if self._labels is None:
            raise ValueError("no label file was given")
        idx = self._index(indices)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self._n):
            raise IndexError(f"index out of range for {self._n} records (negative indices do not wrap)")
        return self._labels[idx]

    def all(self, dtype=torch.float32):
        """Every row in file order: ``take(arange(N))``."""
        return self.take(torch.arange(self._n), dtype=dtype)

    def batches(self, batch_size, shuffle=False, generator=None, drop_last=False, dtype=torch.float32,
                decode_group=65536):
        """Iterate over the dataset in minibatches: yields ``z`` (``[batch_size, z_dim]``, the last one shorter unless
        ``drop_last``), or ``(z, y)`` when the object holds labels.

        ``decode_group`` indices are decoded per launch and the minibatches are VIEWS of that buffer (valid until the
        next group is decoded): one lane decodes one record, a serial chain of ``z_dim`` symbols, so a launch of a few
        hundred records is bound by that chain's latency and leaves most of the chip idle, while 65536 records fill
        it.  The launch is therefore amortised over many minibatches; ``decode_group`` is rounded down to a multiple
        of ``batch_size`` (at least one batch).  The batches do not depend on it.

        With ``shuffle`` the order is ``torch.randperm(N, generator=generator)`` drawn on the CPU, so a seed gives the
        same order whatever device the object lives on."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        order = torch.randperm(self._n, generator=generator) if shuffle else torch.arange(self._n)
        group = max(int(decode_group) // batch_size, 1) * batch_size
        try:
            for g0 in range(0, self._n, group):
                idx = order[g0:g0 + group].to(self.device)
                z = self.take(idx, dtype=dtype)
                y = self._labels[idx] if self._labels is not None else None
                for b0 in range(0, idx.numel(), batch_size):
                    if drop_last and b0 + batch_size > idx.numel():
                        return
                    zb = z[b0:b0 + batch_size]
                    yield zb if y is None else (zb, y[b0:b0 + batch_size])
        finally:
            self.release()     # (working buffers sized by decode_group do not outlive the epoch)

    def release(self):
        """Free whatever working memory the object keeps between ``take`` calls (nothing, here)."""


class CompressedLatents(_Latents):
    """``CompressedLatents(file, compressor, label_file=None, device=None)``

    file         a container written by ``compress_dataset`` (one record per image).
    compressor   the :class:`~lossyless_amd.compressor.ClipCompressor` or
                 :class:`~lossyless_amd.feature_compressor.FeatureCompressor` whose tables coded it; the rows have its
                 ``z_dim`` columns.  Tables too wide for the resident gather kernel are decoded by the windowed one
                 (``lla_rans_decode_gather_wide``), same values.
    label_file   optional ``.npy`` of N labels, kept as an int64 tensor on ``device``.
    device       where the compressed bytes live and the rows are produced; default: the compressor's device.
                 ``"cpu"`` keeps numpy arrays and decodes with the library's host coder (no GPU needed).
    """

    def __init__(self, file, compressor, label_file=None, device=None):
        self._set_device(compressor.device if device is None else device,
                         "CompressedLatents on 'cuda' needs an MI355X (use device='cpu' for the host coder)")
        self.z_dim = int(compressor.z_dim)
        self._n, body, off = _read_container(file)

        t = compressor._tables()
        names = ("cdf", "cdf_len", "offset", "bias", "exp_scale", "median")
        self._W = int(t["W"])
        if self.device.type == "cpu":
            self._body, self._off = body, off
            self._tab = {k: np.ascontiguousarray(t[k].detach().cpu().numpy()) for k in names}
        else:
            self._body = torch.from_numpy(body).to(self.device)
            self._off = torch.from_numpy(off.astype(np.int64)).to(self.device)
            self._tab = {k: t[k].detach().to(self.device).contiguous() for k in names}
        self._load_labels(label_file)

    def _decode(self, idx, B, out, ld, dtype):
        C = self.z_dim
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        L, t = _lib.lib(), self._tab
        if self.device.type == "cpu":
            rc = L.lla_rans_decode_gather_host(
                _np_ptr(self._body), _np_ptr(self._off), 1, self._n, _lib.ptr(idx), B, C, _np_ptr(t["cdf"]), self._W,
                _np_ptr(t["cdf_len"]), _np_ptr(t["offset"]), _np_ptr(t["bias"]), _np_ptr(t["exp_scale"]),
                _np_ptr(t["median"]), _lib.ptr(out), _DTYPES[dtype], ld, _lib.ptr(status))
            _lib.check(rc, "lla_rans_decode_gather_host")
        else:
            head = (_lib.ptr(self._body), _lib.ptr(self._off), 1)
            tail = (self._n, _lib.ptr(idx), B, C, _lib.ptr(t["cdf"]), self._W, _lib.ptr(t["cdf_len"]), _lib.ptr(t["offset"]),
                    _lib.ptr(t["bias"]), _lib.ptr(t["exp_scale"]), _lib.ptr(t["median"]), _lib.ptr(out), _DTYPES[dtype], ld,
                    _lib.ptr(status))
            with torch.cuda.device(self.device):
                if resident_takes(C, self._W, _lib.CODER_GATHER):
                    _lib.check(L.lla_rans_decode_gather(*head, *tail, _lib.stream_ptr(self.device)), "lla_rans_decode_gather")
                else:       # a table too wide to stay in LDS: the windowed kernel, same rows and statuses
                    _lib.check(L.lla_rans_decode_gather_wide(*head, 0, 1, *tail, 0, _lib.stream_ptr(self.device)),
                               "lla_rans_decode_gather_wide")
        return status


class HyperpriorLatents(_Latents):
    """``HyperpriorLatents(file, compressor, label_file=None)``: a hyperprior container (two records per image: z string,
    side string) kept compressed in HBM, with the surface of :class:`CompressedLatents`.

    file         a container written by ``HyperpriorClipCompressor.compress_dataset``.
    compressor   the :class:`~lossyless_amd.hyperprior_compressor.HyperpriorClipCompressor` that coded it, on a GPU: the
                 object lives on its device and reads its ``hyperprior`` module (tables, affine, ``z_encoder``).

    ``take`` is three steps on the current stream, none of which waits for the host: the side records of the named
    images are decoded straight into the zero-padded fp32 input of ``z_encoder``'s first GEMM
    (``lla_rans_decode_gather_strided``: ``float(sym) + median``), the MLP runs on that buffer
    (``MLP.forward_padded``), and ``lla_gaussian_decode_gather`` decodes the z records with the scales the MLP left,
    taking the side pass's statuses as ``status_in``.  Same values, bit for bit, as
    ``decompress_dataset(file)[indices]``.  The coder's mode is the compressor's (``hyperprior.coded_means``): with
    ``"predicted"`` the last step is ``lla_gaussian_decode_gather_means``, which reads the means where the MLP left them
    next to the scales.  The file does not record the mode: opened with a compressor in the other mode (or with another
    state dict) it decodes to wrong values without an error.

    Working memory: besides the compressed bytes (``nbytes``) the object keeps the buffers of the LAST batch length --
    s_hat and the MLP activations, ``workspace_nbytes`` = B x (104 + 512 + 512 + 1024) x 4 bytes, 0.56 GB at B = 65536
    -- so that repeated calls of one length allocate nothing; calls on one object therefore belong on one stream.  A
    call of another length replaces them, ``release()`` frees them, and ``batches()`` releases them when the epoch
    ends.  The tensor returned is never one of them.

    A compressor built with ``mlp_precision="ordered"`` is served the same way (``forward_padded`` then runs
    ``lla_gemm_f32_ordered``).  The object has no host form in either mode: on a CPU compressor it raises, although an
    ordered container itself can be decoded there (``decompress_dataset(file, is_cpu=True)``)."""

    def __init__(self, file, compressor, label_file=None):
        self._set_device(compressor.device, "HyperpriorLatents needs an MI355X")
        if self.device.type != "cuda":
            raise RuntimeError("HyperpriorLatents decodes on the GPU only")
        m = compressor.hyperprior
        if m.mlp_precision not in ("fp32", "ordered"):
            raise NotImplementedError("HyperpriorLatents runs the fp32 and the ordered z_encoder only")
        m._check_device_path("HyperpriorLatents")
        self._model = m
        self.z_dim, self._side_dim = int(m.z_dim), int(m.side_z_dim)
        n_rec, body, off = _read_container(file)
        if n_rec % 2:
            raise ValueError(f"{file}: {n_rec} records, expected two per image")
        self._n = n_rec // 2
        self._body = torch.from_numpy(body).to(self.device)
        self._off = torch.from_numpy(off.astype(np.int64)).to(self.device)
        self._load_labels(label_file)
        self._bufs = None          # (B, s_hat, statuses, activations) of the last batch length

    def _buffers(self, B):
        if self._bufs is None or self._bufs[0] != B:
            kpad, npads = self._model.z_encoder.padded_shapes(self.device)
            # (zeroed once: the gather writes columns [0, side_z_dim) only, the padding columns stay zero)
            s_hat = torch.zeros((B, kpad), dtype=torch.float32, device=self.device)
            status = torch.empty((2, B), dtype=torch.int32, device=self.device)
            acts = [torch.empty((B, n), dtype=torch.float32, device=self.device) for n in npads]
            self._bufs = (B, s_hat, status, acts)
        return self._bufs[1:]

    def release(self):
        """Free the cached working buffers (the next ``take`` allocates them again)."""
        self._bufs = None

    @property
    def workspace_nbytes(self):
        """Bytes of working buffers currently cached (see the class docstring); not part of ``nbytes``."""
        if self._bufs is None:
            return 0
        _, s_hat, status, acts = self._bufs
        return int(s_hat.nbytes + status.nbytes + sum(a.nbytes for a in acts))

    def lds_report(self, dtype=torch.float32):
        """-> dict(granted, front, packed_rows, rows_in_lds): the dynamic LDS a conditional-gather launch asks for on this
        device, the bytes in front of the packed rows, the bytes the rows of this model's table need, and whether the
        kernel therefore searches them in LDS (it falls back to global-memory rows, same values, when they do not fit)."""
        gct = self._model.gaussian_conditional.device_tables()
        T, W = gct["T"], gct["W"]
        front = ctypes.c_size_t(0)
        L = _lib.lib()
        query = (L.lla_gaussian_decode_gather_means_lds_bytes if self._model.coded_means == "predicted"
                 else L.lla_gaussian_decode_gather_lds_bytes)
        with torch.cuda.device(self.device):
            granted = int(query(self.z_dim, T, W, _DTYPES[dtype], ctypes.byref(front)))
        packed = ((T + 1) * 4 + 7) // 8 * 8 + 8 * T + 2 * int(gct["cdf_len"].clamp(3, W).sum())
        return dict(granted=granted, front=int(front.value), packed_rows=packed,
                    rows_in_lds=granted > 0 and int(front.value) + packed <= granted)

    def _decode(self, idx, B, out, ld, dtype):
        m, L = self._model, _lib.lib()
        C, S = self.z_dim, self._side_dim
        p, ebt, gct = m._device_params(), m.entropy_bottleneck.device_tables(), m.gaussian_conditional.device_tables()
        s_hat, status, acts = self._buffers(B)
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            # side records (1, 2): zero bias, unit scale, the medians -> s_hat = float(sym) + median where the GEMM reads it
            rc = L.lla_rans_decode_gather_strided(
                _lib.ptr(self._body), _lib.ptr(self._off), 1, 1, 2, self._n, _lib.ptr(idx), B, S, _lib.ptr(ebt["cdf"]),
                ebt["W"], _lib.ptr(ebt["cdf_len"]), _lib.ptr(ebt["offset"]), _lib.ptr(p["side_bias"]),
                _lib.ptr(p["side_scale"]), _lib.ptr(ebt["median"]), _lib.ptr(s_hat), _lib.LLA_Z_F32, s_hat.shape[1],
                _lib.ptr(status[0]), st)
            _lib.check(rc, "lla_rans_decode_gather_strided")
            params = m.z_encoder.forward_padded(s_hat, acts)
            # z records (0, 2) with row b of the MLP output; a row whose side record failed is not decoded
            head = (_lib.ptr(self._body), _lib.ptr(self._off), 1, 0, 2, self._n, _lib.ptr(idx), B, C, _lib.ptr(p["bias"]),
                    _lib.ptr(p["exp_scale"]), _lib.ptr(params), params.stride(0))
            tail = (_lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]), gct["T"], gct["W"],
                    _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]), _lib.ptr(out), _DTYPES[dtype], ld,
                    _lib.ptr(status[0]), _lib.ptr(status[1]), st)
            if m.coded_means == "predicted":
                _lib.check(L.lla_gaussian_decode_gather_means(*head, m._means_ptr(params), params.stride(0), *tail),
                           "lla_gaussian_decode_gather_means")
            else:
                _lib.check(L.lla_gaussian_decode_gather(*head, *tail), "lla_gaussian_decode_gather")
        return status[1]
