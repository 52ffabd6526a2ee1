"""``FeatureCompressor`` -- the dataset surface of ``ClipCompressor`` for a matrix of features.

``ClipCompressor`` takes images through the CLIP ViT-B/32 tower.  Someone who trained a rate point with
``BottleneckFit`` on the features of ANY frozen encoder (the RN50 tower's 1024 dimensions, a SimCLR / SwAV ResNet's 2048,
the reference's ``bottleneck_rn50simclr_lossyZ`` configs) has a state dict and features, no images and no CLIP weights.
This class is everything behind the tower: the per-dimension affine, the entropy bottleneck, the reference's ``.bin``
container, ``decompress_dataset`` and ``open_dataset``, at the width the state dict has.  The coder is
``EntropyBottleneck.encode_device`` / ``decode_device``: the resident kernels where the table fits them, the windowed
ones (``lla_*_wide``) for every other width.  On ``device="cpu"`` everything runs on the library's host coder, which
writes the same bytes.
"""
import ctypes
import time

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .compressor import ClipCompressor


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def state_dict_z_dim(state_dict):
    """The feature width a factorized rate point was trained at: the length of ``scaling`` (else the bottleneck's
    channel count)."""
    for key, axis in (("scaling", 0), ("biasing", 0), ("entropy_bottleneck.quantiles", 0),
                      ("entropy_bottleneck._quantized_cdf", 0)):
        if key in state_dict:
            return int(state_dict[key].shape[axis])
    raise KeyError("the state dict holds neither `scaling` nor `entropy_bottleneck.*`: not a factorized rate point")


class FeatureCompressor(ClipCompressor):
    """Entropy-bottleneck compressor of feature rows ``[.., z_dim]``: ``ClipCompressor`` without the tower.

    Parameters
    ----------
    pretrained_state_dict : dict or str or Path
        A factorized rate point -- ``BottleneckFit(...).fit(Z).state_dict()``, the reference's ``HRateFactorizedPrior``,
        the shipped ``*_factorized_rate.pt`` -- or a path to one.  ``z_dim`` is read from it.
    device : str
        ``"cuda"`` (an MI355X) or ``"cpu"`` (the library's host coder: same bytes, same values).

    ``compressor(Z) -> Z_hat``, ``compress(Z) -> list of bytes``, ``decompress(strings)``, ``get_rate(Z)``,
    ``compress_dataset(Z, file, ...)``, ``decompress_dataset(file, ...)``, ``open_dataset(file, ...)``.  ``Z`` is fp16
    or fp32 (anything else is converted to fp32) and is quantised from the values as given; a row of another width is a
    ``ValueError``.  For the same rows and state dict at 512 dimensions the file is ``ClipCompressor``'s, byte for byte.
    """

    def __init__(self, pretrained_state_dict, device="cuda" if torch.cuda.is_available() else "cpu"):
        nn.Module.__init__(self)     # (ClipCompressor's own constructor builds the tower first)
        if not isinstance(pretrained_state_dict, dict):
            pretrained_state_dict = torch.load(pretrained_state_dict, map_location="cpu", weights_only=True)
        self.z_dim = state_dict_z_dim(pretrained_state_dict)
        self.clip = self.preprocess = None
        self._init_rate_model(pretrained_state_dict, device)

    # ------------------------------------------------------------------ features in
    def _on_host(self):
        return str(self.device) == "cpu"

    def _features(self, Z):
        """-> contiguous [B, z_dim] fp16 / fp32 tensor on ``self.device``."""
        if not isinstance(Z, torch.Tensor):
            Z = torch.as_tensor(np.asarray(Z))
        if Z.dim() != 2 or Z.shape[1] != self.z_dim:
            got = tuple(Z.shape)
            raise ValueError(f"expected rows of width {self.z_dim} (the state dict's z_dim), got width "
                             f"{got[-1] if got else 'none'} (shape {got})")
        if Z.dtype not in (torch.float16, torch.float32):
            Z = Z.float()
        return Z.to(self.device).contiguous()

    def _embed(self, Z):
        self._check_gpu()
        return self._features(Z)

    # ------------------------------------------------------------------ host coder
    def _host_tables(self):
        t = self._tables()
        return {k: (np.ascontiguousarray(v.detach().cpu().numpy()) if hasattr(v, "cpu") else v) for k, v in t.items()}

    def _symbols_host(self, z, t):
        """lla_quantise on the host: three separately rounded fp32 operations, round-half-even."""
        y = (z.float() + torch.from_numpy(t["bias"])) * torch.from_numpy(t["exp_scale"])
        return np.ascontiguousarray(torch.round(y - torch.from_numpy(t["median"])).to(torch.int32).numpy())

    def _encode_host(self, z, record_prefix):
        """Rows on the host -> (streams back to back as a uint8 array, be32-prefixed if asked; offsets uint64 [B + 1])."""
        t = self._host_tables()
        sym = self._symbols_host(z, t)
        B, C = sym.shape
        off = np.zeros(B + 1, dtype=np.uint64)
        L = _lib.lib()
        args = (_np_ptr(sym), B, C, _np_ptr(t["cdf"]), t["W"], _np_ptr(t["cdf_len"]), _np_ptr(t["offset"]),
                1 if record_prefix else 0)
        rc = L.lla_rans_encode_batch_host(*args, None, 0, _np_ptr(off))      # sizes first (LLA_ECAP: as documented)
        if rc not in (_lib.LLA_OK, _lib.LLA_ECAP):
            _lib.check(rc, "lla_rans_encode_batch_host")
        out = np.empty(max(int(off[-1]), 1), dtype=np.uint8)
        _lib.check(L.lla_rans_encode_batch_host(*args, _np_ptr(out), out.size, _np_ptr(off)), "lla_rans_encode_batch_host")
        return out[:int(off[-1])], off

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def forward(self, Z, is_compress=False):
        """Z [B, z_dim] -> Z_hat [B, z_dim] fp32 on ``self.device``, or the list of byte strings if ``is_compress``."""
        if not self._on_host():
            return super().forward(Z, is_compress)
        z = self._features(Z)
        if is_compress:
            blob, off = self._encode_host(z, record_prefix=False)
            blob = blob.tobytes()
            return [blob[int(off[i]):int(off[i + 1])] for i in range(z.shape[0])]
        t = self._host_tables()
        sym = self._symbols_host(z, t)
        out = np.empty(sym.shape, dtype=np.float32)
        rc = _lib.lib().lla_dequantise_host(_np_ptr(sym), sym.shape[0], sym.shape[1], _np_ptr(t["bias"]),
                                            _np_ptr(t["exp_scale"]), _np_ptr(t["median"]), _np_ptr(out))
        _lib.check(rc, "lla_dequantise_host")
        return torch.from_numpy(out)

    # ------------------------------------------------------------------ datasets
    def _groups(self, Z, rows):
        """Z (a [N, z_dim] tensor or an iterable of [b, z_dim] batches) -> checked pieces of at most ``rows`` rows each,
        small batches gathered; records do not depend on their neighbours, so any grouping gives the same file."""
        if isinstance(Z, (torch.Tensor, np.ndarray)):
            Z = (Z,)
        held, n = [], 0
        for batch in Z:
            z = self._features(batch)
            for i in range(0, z.shape[0], rows):
                piece = z[i:i + rows]
                if held and (held[0].dtype != piece.dtype or n + piece.shape[0] > rows):
                    yield torch.cat(held) if len(held) > 1 else held[0]
                    held, n = [], 0
                held.append(piece)
                n += piece.shape[0]
        if held:
            yield torch.cat(held) if len(held) > 1 else held[0]

    @torch.no_grad()
    def compress_dataset(self, Z, file, label_file=None, labels=None, is_info=True, *, entropy_group=16):
        """Code the rows of ``Z`` -- a ``[N, z_dim]`` tensor or an iterable of ``[b, z_dim]`` batches, fp16 or fp32, on any
        device -- into the reference's container ``file`` (hub/compressor.py:192-207: what ``ClipCompressor`` writes),
        ``entropy_group`` x 1024 rows per launch sequence with one device->host sync each.  ``labels`` (N integers) are
        saved to ``label_file`` as the reference saves them."""
        if (label_file is None) != (labels is None):
            raise ValueError("`labels` and `label_file` go together")
        start = time.time()
        rows = max(int(entropy_group), 1) * 1024
        out, n = [], 0
        for z in self._groups(Z, rows):
            if self._on_host():
                out.append(self._encode_host(z, record_prefix=True)[0])
            else:
                payload, offsets = self._encode_records(z)
                out.append(payload[:int(offsets[-1])].cpu().numpy())
            n += z.shape[0]
        if labels is not None:
            labels = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.uint16)
            if labels.shape != (n,):
                raise ValueError(f"{labels.shape[0] if labels.ndim else 0} labels for {n} rows")
        body = np.concatenate(out) if out else np.zeros(0, np.uint8)
        self._write_container(file, body, n, labels, label_file, start, is_info)
