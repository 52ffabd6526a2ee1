"""``HyperpriorClipCompressor`` -- ``ClipCompressor``'s dataset interface over the scale-hyperprior coder.

The reference's headline rates come from ``HRateHyperprior`` (lossyless/rates.py:572-756), but its hub only ships the
factorized model (hub/compressor.py).  This class puts the hyperprior behind the same surface -- ``compressor(X)``,
``compress``, ``decompress``, ``get_rate``, ``compress_dataset``, ``decompress_dataset`` -- for a state dict trained with
the reference's ``main.py``.  The tower, the prefetch and the :class:`~lossyless_amd.compressor.RecordStream` pipeline are
``ClipCompressor``'s; a group of embeddings is coded by ``HRateHyperprior.encode_device`` (side encoder -> fused quantise +
rANS of the side information -> z_encoder -> ``lla_gaussian_quantise_encode`` -> ``lla_rans_compact_pairs``) without
leaving the device.

The file is the reference's framing (hub/compressor.py:192-196, :233-237) with TWO records per image: ``be32(2N)``, then
records ``2i`` (z string) and ``2i+1`` (side string) of image ``i`` -- ``read_uints`` / ``read_bytes`` and
``lla_container_index`` walk it unchanged.
"""
import ctypes
import io
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .compressor import ClipCompressor, read_bytes, read_uints, write_bytes, write_uints
from .rates import HRateHyperprior

_WHY_NO_CPU = ("the coding-table row of every element is chosen by the z_encoder MLP, which runs on the fp32 MFMA GEMM "
               "(lla_gemm_f32); a CPU evaluation of the MLP is roundoff-close but not bit-equal (another summation order), so "
               "it may pick other rows and decode garbage: strings written on the GPU are decoded on the GPU (see "
               "lossyless_amd.rates.MLP). Use is_cpu=False.")


def write_pair_container(file, z_strings, side_strings):
    """Write ``be32(2N)`` + records ``z_0, side_0, z_1, ...`` (each ``be32(len)`` + bytes) to a path or a binary file
    object, with the reference's field writers."""
    if len(z_strings) != len(side_strings):
        raise ValueError("one side string per z string expected")
    if not hasattr(file, "write"):
        with Path(file).open("wb") as f:
            return write_pair_container(f, z_strings, side_strings)
    write_uints(file, (2 * len(z_strings),))
    for pair in zip(z_strings, side_strings):
        for s in pair:
            write_uints(file, (len(s),))
            write_bytes(file, s)


def read_pair_container(file):
    """Inverse of :func:`write_pair_container` (the reference's reader loop, hub/compressor.py:233-237, two records per
    image) -> ``[z_strings, side_strings]``.  ValueError on an odd record count or a file that ends early."""
    if not hasattr(file, "read"):
        with Path(file).open("rb") as f:
            return read_pair_container(f)

    def uint():
        raw = file.read(4)       # (read_uints would turn a short read into a smaller number)
        if len(raw) != 4:
            raise ValueError("pair container ends inside a record")
        return read_uints(io.BytesIO(raw), 1)[0]

    n = uint()
    if n % 2:
        raise ValueError(f"pair container holds an odd number of records ({n})")
    out = [[], []]
    for r in range(n):
        length = uint()
        s = read_bytes(file, length)
        if len(s) != length:
            raise ValueError("pair container ends inside a record")
        out[r % 2].append(s)
    return out


def _pair_records(z_strings, side_strings):
    """-> (record bytes as uint8 numpy, padded by a word for the decoders; int64 offsets [2B+1])."""
    if len(z_strings) != len(side_strings):
        raise ValueError("one side string per z string expected")
    parts, off = [], np.zeros(2 * len(z_strings) + 1, dtype=np.int64)
    for i, pair in enumerate(zip(z_strings, side_strings)):
        for k, s in enumerate(pair):
            parts += [len(s).to_bytes(4, "big"), bytes(s)]
            off[2 * i + k + 1] = off[2 * i + k] + 4 + len(s)
    return np.frombuffer(b"".join(parts) + b"\0\0\0\0", dtype=np.uint8), off


class HyperpriorClipCompressor(ClipCompressor):
    """CLIP ViT-B/32 + scale-hyperprior compressor: the surface of :class:`ClipCompressor`, the coder of
    :class:`~lossyless_amd.rates.HRateHyperprior` (``self.hyperprior``).

    Parameters
    ----------
    pretrained_state_dict : dict or str or Path
        What the reference's ``HRateHyperprior`` saves (``scaling``, ``biasing``, ``entropy_bottleneck.*``,
        ``gaussian_conditional.*``, ``side_encoder.*``, ``z_encoder.*``), or a path to it; loaded by
        ``HRateHyperprior._load_from_state_dict``.  Coding tables the state dict carries are kept, missing ones built.
    is_jit, device, clip_weights, vit_chunk, gpu_preprocess
        As for :class:`ClipCompressor`.  ``"cpu"`` builds the module; every compute entry point raises.
    coded_means : ``"scales"`` (default) or ``"predicted"``
        Passed to :class:`~lossyless_amd.rates.HRateHyperprior`: the reference's coder (the scales stand in for the means),
        or the opt-in one that codes with the predicted means the likelihood was trained with.  ``forward``, ``compress``,
        ``decompress``, ``get_rate``, ``compress_dataset``, ``decompress_dataset`` and ``open_dataset`` all follow it.  The
        container format is the same in both modes and does not record the mode: a file written in one and read in the
        other -- like a file read with another state dict -- decodes to wrong values without an error.
    mlp_precision : ``"fp32"`` (default), ``"fp16"`` or ``"ordered"``
        Passed to :class:`~lossyless_amd.rates.HRateHyperprior`: which arithmetic the two hyperprior MLPs run in.  With
        ``"ordered"`` (every MLP output one ascending ``fmaf`` chain, on a VALU kernel) the host reproduces the GPU's table
        rows bit for bit, so ``decompress_dataset(file, is_cpu=True)`` decodes on the host -- on this compressor or on one
        built with ``device="cpu"`` -- and ``decompress(strings)`` works on a CPU compressor; ``compress_dataset``,
        ``compress`` and ``forward`` still need the GPU (the tower has no CPU path), and ``open_dataset`` on the CPU keeps
        raising.  Like ``coded_means`` the mode is neither in the container nor in ``state_dict()``, and combines freely
        with it: a file written in one mode and read in another decodes to wrong values without an error.

    ``compress(X)`` returns ``[z_strings, side_z_strings]`` (what ``HRateHyperprior.compress`` returns), ``decompress``
    takes it back.  ``compressor(X)`` is the coded representation without coding and equals ``decompress(compress(X))``
    bit for bit.  ``decompress_dataset`` decodes on the GPU only: ``is_cpu`` defaults to False here and ``is_cpu=True``
    raises ``NotImplementedError`` unless ``mlp_precision="ordered"``, because the table rows are chosen by the fp32 MFMA
    MLP, which a CPU evaluation reproduces to roundoff but not bit for bit -- strings written here are decoded here.
    """

    records_per_image = 2

    def __init__(self, pretrained_state_dict, is_jit=False,
                 device="cuda" if torch.cuda.is_available() else "cpu", *,
                 clip_weights=None, vit_chunk=0, gpu_preprocess=False, coded_means="scales",
                 mlp_precision="fp32"):
        nn.Module.__init__(self)     # (ClipCompressor's own constructor goes on to build the factorized model)
        self._init_tower(clip_weights, vit_chunk, gpu_preprocess)
        if not isinstance(pretrained_state_dict, dict):
            pretrained_state_dict = torch.load(pretrained_state_dict, map_location="cpu", weights_only=True)
        side_w = pretrained_state_dict.get("side_encoder.module.8.weight")
        self.hyperprior = HRateHyperprior(self.z_dim, side_z_dim=None if side_w is None else int(side_w.shape[0]),
                                          coded_means=coded_means, mlp_precision=mlp_precision)
        self.side_z_dim = self.hyperprior.side_z_dim
        missing, _ = self.hyperprior.load_state_dict(pretrained_state_dict, strict=False)
        tables = ("_quantized_cdf", "_offset", "_cdf_length", "scale_table")     # (built below when not carried)
        missing = [k for k in missing if k.rsplit(".", 1)[-1] not in tables]
        if missing:
            raise KeyError(f"not a HRateHyperprior state dict: {sorted(missing)[:4]} ... missing")
        self.hyperprior.update()     # no-op for tables the state dict carried

        self.device = device
        self.to(self.device)
        self.eval()

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def forward(self, X, is_compress=False):
        """``[z_strings, side_z_strings]`` if ``is_compress`` else z_hat [B,512] fp32 on the GPU.  Returning ``bytes``
        costs one host sync per call (offsets and payload are copied out); ``compress_dataset`` does not go through here."""
        z = self._embed(X)
        if not is_compress:
            return self.hyperprior.represent_device(z)
        B = z.shape[0]
        payload, offsets = self.hyperprior.encode_device(z)
        off = offsets.cpu().numpy()
        blob = payload[: int(off[-1])].cpu().numpy().tobytes()
        rec = [blob[int(off[r]) + 4:int(off[r + 1])] for r in range(2 * B)]
        return [rec[0::2], rec[1::2]]

    def process_z_in(self, z):
        return self.hyperprior.process_z_in(z)

    def process_z_out(self, z_hat):
        return self.hyperprior.process_z_out(z_hat)

    @torch.no_grad()
    def decompress(self, all_strings):
        """``[z_strings, side_z_strings]`` -> z_hat [B,512] fp32 on the GPU (one host sync per call: ``decode_device``
        reads the statuses back before it returns)."""
        on_host = self._ordered and str(self.device) == "cpu"      # (ordered: a CPU compressor decodes on the host)
        if not on_host:
            self._check_gpu()
        if not (isinstance(all_strings, (list, tuple)) and len(all_strings) == 2):
            raise ValueError("expected [z_strings, side_z_strings]")
        body, off = _pair_records(*all_strings)
        if on_host:
            return torch.from_numpy(self._decode_records_host(body, off, len(all_strings[0])))
        return self._decode_records(body, off, len(all_strings[0]))

    def get_rate(self, X):
        """Mean coded size per image in bits, both strings counted."""
        z_strings, side_strings = self.compress(X)
        return 8 * (sum(map(len, z_strings)) + sum(map(len, side_strings))) / len(z_strings)

    # ------------------------------------------------------------------ records
    def _encode_records(self, z):
        return self.hyperprior.encode_device(z)

    def _decode_records(self, body, off_np, B):
        """body: uint8 numpy of 2B records (+ at least 4 spare bytes); off_np [2B+1] -> fp32 [B,512] device tensor."""
        dev = torch.device(self.device)
        payload = torch.from_numpy(np.ascontiguousarray(body)).to(dev)
        offsets = torch.from_numpy(np.ascontiguousarray(off_np).astype(np.int64)).to(dev)
        try:
            return self.hyperprior.decode_device(payload, offsets, B)
        except ValueError as e:
            raise ValueError(f"{e} in container") from None

    def _decode_strings(self, strings):
        return self.decompress(strings)

    # What ClipCompressor keeps for its factorized model and its host decoder has no counterpart here.
    def _tables(self):
        raise NotImplementedError("HyperpriorClipCompressor has no factorized coding tables (scaling / biasing / "
                                  "entropy_bottleneck live in self.hyperprior)")

    @staticmethod
    def _records_of(strings):
        raise NotImplementedError("HyperpriorClipCompressor codes two records per image: see decompress")

    @property
    def _ordered(self):
        return self.hyperprior.mlp_precision == "ordered"

    def _decode_records_host(self, body, off_np, B):
        """Host twin of ``_decode_records`` (``HRateHyperprior.decode_host``) -> float32 [B,512] ndarray, no GPU involved;
        ``mlp_precision="ordered"`` only."""
        if not self._ordered:
            raise NotImplementedError("HyperpriorClipCompressor has no host decoder: " + _WHY_NO_CPU)
        payload = torch.from_numpy(np.array(body, dtype=np.uint8))      # (a copy: the caller's may be read-only)
        offsets = torch.from_numpy(np.ascontiguousarray(off_np).astype(np.int64))
        try:
            return self.hyperprior.decode_host(payload, offsets, B).numpy()
        except ValueError as e:
            raise ValueError(f"{e} in container") from None

    # ------------------------------------------------------------------ datasets
    def open_dataset(self, file, label_file=None, device=None):
        """The container ``file`` as a :class:`~lossyless_amd.latents.HyperpriorLatents`: it stays compressed in HBM and
        serves the rows of any index vector, bit-equal to ``decompress_dataset(file)[indices]``.  GPU only: the object
        always lives on this compressor's device (it reads the compressor's tables and MLP there; ``device`` only says
        GPU or CPU); ``device="cpu"``, or a compressor on the CPU, raises ``NotImplementedError`` before the file is
        touched -- with ``mlp_precision="ordered"`` too: ``HyperpriorLatents`` has no host form."""
        here = torch.device(self.device)
        want = here if device is None else torch.device(device)
        if here.type != "cuda" or want.type != "cuda":
            raise NotImplementedError(
                "HyperpriorClipCompressor.open_dataset on the CPU: a hyperprior container holds two records per image (z "
                "string, side string), and a z record can only be decoded with the table rows and means that z_encoder "
                "derives from its decoded side record; " + _WHY_NO_CPU)
        from .latents import HyperpriorLatents
        return HyperpriorLatents(file, self, label_file=label_file)

    @torch.no_grad()
    def decompress_dataset(self, file, label_file=None, is_info=True, is_cpu=False, *, batch_size=65536):
        """Decompress a file written by ``compress_dataset`` -> float32 [N,512] ndarray (and the labels).

        ``is_cpu=True`` raises ``NotImplementedError``: the table rows are chosen by the fp32 MFMA MLP, and a CPU
        evaluation of it is roundoff-close, not bit-equal, so it may pick other rows -- unless the compressor was built with
        ``mlp_precision="ordered"``: then the records are decoded on the host (``HRateHyperprior.decode_host``), on a
        compressor on either device, to the array ``is_cpu=False`` gives, bit for bit.  ``batch_size`` images are decoded
        per launch; any value gives the same array.  ValueError for a file that is truncated, holds an odd number of
        records or a damaged record."""
        if is_cpu and not self._ordered:
            raise NotImplementedError("HyperpriorClipCompressor.decompress_dataset(is_cpu=True): " + _WHY_NO_CPU)
        if not is_cpu:
            self._check_gpu()
        start = time.time()
        blob = np.fromfile(str(file), dtype=np.uint8)
        L = _lib.lib()
        n = ctypes.c_uint32(0)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        # (validates the count against the file size before anything is sized by it)
        rc = L.lla_container_index(P(blob), blob.size, None, 0, ctypes.byref(n)) if blob.size >= 4 else _lib.LLA_EDATA
        off = np.zeros(int(n.value) + 1, dtype=np.uint64)
        if rc == _lib.LLA_OK:
            rc = L.lla_container_index(P(blob), blob.size, P(off), off.size, ctypes.byref(n))
        if rc == _lib.LLA_EDATA:
            raise ValueError(f"{file}: truncated or malformed container")
        _lib.check(rc, "lla_container_index")
        if n.value % 2:
            raise ValueError(f"{file}: {n.value} records, expected two per image")
        n_img = int(n.value) // 2
        body = np.concatenate([blob[4:], np.zeros(4, np.uint8)])     # (the decoders read whole words)

        Z_hat = np.empty((n_img, self.z_dim), dtype=np.float32)
        for i in range(0, n_img, batch_size):
            j = min(i + batch_size, n_img)
            b0, b1 = int(off[2 * i]), int(off[2 * j])
            args = (body[b0:b1 + 4], off[2 * i:2 * j + 1] - off[2 * i], j - i)
            Z_hat[i:j] = self._decode_records_host(*args) if is_cpu else self._decode_records(*args).cpu().numpy()

        dec_time = (time.time() - start) / max(n_img, 1)
        if is_info:
            print(f"Decoding: {1/dec_time:.2f} img/sec ")
        if label_file is not None:
            return Z_hat, np.load(label_file, allow_pickle=False).astype(np.int64)
        return Z_hat
