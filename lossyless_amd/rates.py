"""Training-side twin of the hub compressor's coder: ``HRateFactorizedPrior`` / ``HRateHyperprior``.

Mirror of the inference-time surface of ``lossyless/rates.py`` that the reference's evaluator drives
(``learnable_compressors.py:84`` ``make_pickable_``, ``:161-163,190`` ``compress`` / ``__call__``, ``:341``
``prepare_compressor_``, ``:436`` ``make_pickable_``): ``RateEstimator`` :77-314 (``forward`` ->
``forward_help`` -> ``(z_hat, rates, logs, other)``, ``real_rate``, ``make_pickable_`` / ``undo_pickable_``,
``update``, ``prepare_compressor_``), ``HRateEstimator`` :398-506 (``scaling/biasing``, ``process_z_in/out``
:434-438, the CDF-buffer-aware load hook :440-473, ``is_coder_updated / is_coder_present /
is_compute_real_rate`` :482-506), ``HRateFactorizedPrior`` :509-564 and ``HRateHyperprior`` :572-756 -- so that
``LearnableCompressor`` can evaluate and code representations with the HIP kernels.  Training ``HRateFactorizedPrior`` on
frozen features (noise, the auxiliary loss, both optimisers) is ``lossyless_amd.BottleneckFit`` (bottleneck_fit.py).
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _lib
from .entropy import EntropyBottleneck, _require_coder, update_registered_buffers


BASE_LOG = 2   # lossyless/helpers.py:27


def _entropy_models(module):
    from .entropy import GaussianConditional
    return [m for m in module.modules() if isinstance(m, (EntropyBottleneck, GaussianConditional))]


class RateEstimator(nn.Module):
    """lossyless/rates.py:77-314 (base class of the coders), inference-time part."""

    is_can_compress = False

    def __init__(self, z_dim, warmup_k_epoch=0, is_endToEnd=True):
        super().__init__()
        self.z_dim = z_dim
        self.warmup_k_epoch = warmup_k_epoch
        self.is_endToEnd = is_endToEnd

    def forward(self, z, p_Zlx, parent=None):
        """rates.py:104-146 -> ``(z_hat, rates [batch], logs, other)``; fp32 whatever autocast says."""
        with torch.autocast(device_type=z.device.type, enabled=False):
            z_hat, rates, r_logs, r_other = self.forward_help(z, p_Zlx, parent)
            epoch = getattr(parent, "current_epoch", self.warmup_k_epoch)
            if (not self.is_endToEnd) or (epoch < self.warmup_k_epoch):
                # disjoint training / warm-up (rates.py:136-144): the rate is recomputed on detached inputs
                z_detached = z.detach() + z * 0
                p_detached = p_Zlx.detach(is_grad_flow=True) if p_Zlx is not None else None
                _, rates, *_ = self.forward_help(z_detached, p_detached, parent)
        return z_hat, rates, r_logs, r_other

    def forward_help(self, z, p_Zlx, parent=None):
        raise NotImplementedError()

    def compress(self, z, parent=None):
        raise NotImplementedError()

    def decompress(self, all_strings):
        raise NotImplementedError()

    def real_rate(self, z, is_return_logs=False, parent=None):
        """rates.py:215-260: mean coded bits per example (sum over latents, mean over batch);
        with ``is_return_logs`` also the reference's log dict -- ``compress_time`` and
        ``receiver_time`` in seconds per example (rates.py:241-257), ``n_bits``."""
        import time
        batch = z.shape[0]
        dev = z.device if z.is_cuda else None

        def clock():
            if dev is not None:
                torch.cuda.synchronize(dev)
            return time.perf_counter()

        t0 = clock()
        all_strings = self.compress(z, parent=parent)
        t1 = clock()
        if is_return_logs:
            _ = self.decompress(all_strings)
            t2 = clock()
        n_bytes = sum(sum(len(s) for s in strings) / len(strings) for strings in all_strings)
        n_bits = n_bytes * 8
        if is_return_logs:
            logs = dict(compress_time=(t1 - t0) / batch, receiver_time=(t2 - t1) / batch,
                        n_bits=n_bits)
            return n_bits, logs
        return n_bits

    def make_pickable_(self):
        """rates.py:273-277: detach the coder objects (the reference's are pybind11 handles that do not pickle;
        ``LearnableCompressor`` calls this right after construction and after the test epoch,
        learnable_compressors.py:84,436).  ``is_coder_present`` turns False, ``compress`` refuses."""
        for m in _entropy_models(self):
            m.entropy_coder = None

    def undo_pickable_(self):
        """rates.py:279-284."""
        from .entropy import HipEntropyCoder
        for m in _entropy_models(self):
            m.entropy_coder = HipEntropyCoder()

    def update(self, force=False):
        """rates.py:286-305: (re)build the integer tables of every entropy model; True if all changed."""
        from .entropy import GaussianConditional
        updated = True
        for m in self.children():
            if isinstance(m, EntropyBottleneck):
                updated &= bool(m.update(force=force))
            elif isinstance(m, GaussianConditional):
                updated &= bool(m.update_scale_table(get_scale_table(), force=force))
        return updated

    def prepare_compressor_(self):
        """rates.py:307-314: coder attached, tables rebuilt."""
        self.undo_pickable_()
        self.update(force=True)


class HRateEstimator(RateEstimator):
    """lossyless/rates.py:398-506: per-dimension affine in front of the entropy models + coder state."""

    is_can_compress = True

    def __init__(self, z_dim, kwargs_ent_bottleneck={}, **kwargs):
        super().__init__(z_dim, **kwargs)
        self.kwargs_ent_bottleneck = dict(kwargs_ent_bottleneck)
        self.scaling = torch.nn.Parameter(torch.ones(z_dim))
        self.biasing = torch.nn.Parameter(torch.zeros(z_dim))

    def _exp_scaling(self):
        """exp(scaling) as the coding tables hold it (``EntropyBottleneck.device_tables``): evaluated in float64,
        rounded once to fp32 -- so ``forward`` quantises exactly where ``compress`` does."""
        return torch.exp(self.scaling.double()).float()

    # rates.py:434-438
    def process_z_in(self, z):
        return (z.float() + self.biasing) * self._exp_scaling()

    def process_z_out(self, z_hat):
        return (z_hat / self._exp_scaling()) - self.biasing

    # rates.py:440-473: the CDF buffers have data-dependent sizes
    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        try:
            update_registered_buffers(self.entropy_bottleneck, f"{prefix}entropy_bottleneck",
                                      ["_quantized_cdf", "_offset", "_cdf_length"], state_dict,
                                      policy="resize")
        except KeyError:
            pass
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @property
    def is_coder_updated(self):
        """rates.py:482-490."""
        return all(m._offset.numel() > 0 for m in _entropy_models(self))

    @property
    def is_coder_present(self):
        """rates.py:492-500."""
        return all(m.entropy_coder is not None for m in _entropy_models(self))

    @property
    def is_compute_real_rate(self):
        """rates.py:502-506."""
        return (not self.training) and self.is_coder_updated and self.is_coder_present

    def _add_real_rate(self, z, logs):
        """The tail both ``forward_help`` share (rates.py:542-545, :668-671)."""
        if self.is_compute_real_rate:
            n_bits, logs2 = self.real_rate(z, is_return_logs=True)
            logs.update(logs2)
            logs["n_bits"] = n_bits


class HRateFactorizedPrior(HRateEstimator):
    """z [B, z_dim] -> one rANS stream per row, same bytes as ``ClipCompressor.compress``.

    ``compress`` returns ``[strings]`` (a list holding the list of byte strings: the
    reference keeps the outer list "for generality when hyperprior", rates.py:556-559)."""

    def __init__(self, z_dim, **kwargs):
        super().__init__(z_dim, **kwargs)
        self.entropy_bottleneck = EntropyBottleneck(z_dim, **self.kwargs_ent_bottleneck)

    def forward_help(self, z, _, parent=None):
        """rates.py:534-554 (eval mode): ``z_hat`` = dequantised representation, ``-log q(z)`` per example in
        nats, logs ``H_q_Z`` (bits), ``H_ZlX`` and -- when the coder is usable -- the real rate's
        ``n_bits / compress_time / receiver_time``."""
        z_in = self.process_z_in(z)
        z_hat, q_z = self.entropy_bottleneck(z_in)
        neg_log_q_z = -torch.log(q_z).sum(-1)
        logs = dict(H_q_Z=neg_log_q_z.mean() / math.log(BASE_LOG), H_ZlX=0)
        self._add_real_rate(z, logs)
        other = dict()
        z_hat = self.process_z_out(z_hat)
        return z_hat, neg_log_q_z, logs, other

    def _tables(self):
        return self.entropy_bottleneck.device_tables(self.scaling, self.biasing)

    @torch.no_grad()
    def compress(self, z, parent=None):
        """rates.py:556-559.  z [B, z_dim] on the GPU (fp16 or fp32)."""
        if not self.is_coder_updated:
            raise RuntimeError("call update() / prepare_compressor_() first")
        _require_coder(self.entropy_bottleneck)
        z = z.contiguous()
        if z.dtype not in (torch.float16, torch.float32):
            z = z.float()
        if not z.is_cuda:
            return [self._compress_host(z)]
        payload, offsets, _ = self.entropy_bottleneck.encode_device(z, self._tables())
        off = offsets.cpu().numpy()
        blob = payload[: int(off[-1])].cpu().numpy().tobytes()
        return [[blob[int(off[i]):int(off[i + 1])] for i in range(z.shape[0])]]

    @torch.no_grad()
    def decompress(self, all_strings):
        """rates.py:561-564 -> z_hat [B, z_dim] fp32 on the GPU."""
        assert isinstance(all_strings, list) and len(all_strings) == 1
        _require_coder(self.entropy_bottleneck)
        strings = all_strings[0]
        import numpy as np
        if self.scaling.device.type != "cuda":
            return self._decompress_host(strings)
        B = len(strings)
        lens = np.fromiter((len(s) for s in strings), dtype=np.int64, count=B)
        off = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        dev = self.scaling.device
        blob = np.frombuffer(b"".join(strings) + b"\0\0\0\0", dtype=np.uint8).copy()
        tables = self._tables()
        sym, status = self.entropy_bottleneck.decode_device(
            torch.from_numpy(blob).to(dev), torch.from_numpy(off).to(dev), B, tables)
        if B and int(status.max()) != 0:
            raise ValueError("malformed rANS stream")
        out = torch.empty((B, self.z_dim), dtype=torch.float32, device=dev)
        rc = _lib.lib().lla_dequantise(_lib.ptr(sym), B, self.z_dim, _lib.ptr(tables["bias"]),
                                       _lib.ptr(tables["exp_scale"]), _lib.ptr(tables["median"]),
                                       _lib.ptr(out), _lib.stream_ptr(dev))
        _lib.check(rc, "lla_dequantise")
        return out


    # ---- a module on the CPU codes with the library's HOST coder (the reference's coder runs on the CPU
    # wherever the module lives): same symbols (three separately rounded fp32 operations, round-half-even),
    # same strings as the device kernels
    def _host_tables(self):
        import numpy as np
        t = self._tables()
        return {k: (np.ascontiguousarray(v.cpu().numpy()) if hasattr(v, "cpu") else v) for k, v in t.items()}

    def _compress_host(self, z):
        import ctypes
        import numpy as np
        t = self._host_tables()
        zf = z.float()
        y = (zf + torch.from_numpy(t["bias"])) * torch.from_numpy(t["exp_scale"])
        sym = np.ascontiguousarray(torch.round(y - torch.from_numpy(t["median"])).to(torch.int32).numpy())
        B, C = sym.shape
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        off = np.zeros(B + 1, dtype=np.uint64)
        L = _lib.lib()
        args = (P(sym), B, C, P(t["cdf"]), t["W"], P(t["cdf_len"]), P(t["offset"]), 0)
        rc = L.lla_rans_encode_batch_host(*args, None, 0, P(off))
        if rc not in (_lib.LLA_OK, -2):
            _lib.check(rc, "lla_rans_encode_batch_host")
        out = np.empty(max(int(off[-1]), 1), dtype=np.uint8)
        _lib.check(L.lla_rans_encode_batch_host(*args, P(out), out.size, P(off)), "lla_rans_encode_batch_host")
        blob = out.tobytes()
        return [blob[int(off[i]):int(off[i + 1])] for i in range(B)]

    def _decompress_host(self, strings):
        import ctypes
        import numpy as np
        t = self._host_tables()
        B, C = len(strings), self.z_dim
        lens = np.fromiter((len(s) for s in strings), dtype=np.uint64, count=B)
        off = np.zeros(B + 1, dtype=np.uint64)
        np.cumsum(lens, out=off[1:])
        blob = np.frombuffer(b"".join(strings) + b"\0\0\0\0", dtype=np.uint8).copy()
        sym = np.empty((B, C), dtype=np.int32)
        status = np.zeros(max(B, 1), dtype=np.int32)
        out = np.empty((B, C), dtype=np.float32)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        L = _lib.lib()
        _lib.check(L.lla_rans_decode_batch_host(P(blob), P(off), 0, B, C, P(t["cdf"]), t["W"], P(t["cdf_len"]),
                                                P(t["offset"]), P(sym), P(status)), "lla_rans_decode_batch_host")
        if B and int(status.max()) != 0:
            raise ValueError("malformed rANS stream")
        _lib.check(L.lla_dequantise_host(P(sym), B, C, P(t["bias"]), P(t["exp_scale"]), P(t["median"]), P(out)),
                   "lla_dequantise_host")
        return torch.from_numpy(out)


def get_scale_table(min=0.11, max=256, levels=64):
    """rates.py:567-569."""
    return torch.exp(torch.linspace(math.log(min), math.log(max), levels))


class MLP(nn.Module):
    """The reference's ``MLP`` (lossyless/architectures.py:94-168) in the configuration the
    hyperprior uses it (identity norm, ReLU, no dropout): same ``module`` Sequential layout, so
    its state-dict keys (``module.0.weight`` ... ) load unchanged.

    On the GPU the layers run on the library's fp32 matrix-core GEMM (``lla_gemm_f32``:
    ``v_mfma_f32_32x32x2_f32``, fp32 operands and accumulation, bias + ReLU in the epilogue) -- the
    reference evaluates these networks in fp32 under ``autocast(False)`` (lossyless/rates.py:104: "precision here
    is important"), and the scale indexes they produce select the coding tables, i.e. they are part of the
    bitstream's contract.  The K order of every output element is fixed by the kernel, so the values do not depend
    on the batch size (a decoder may evaluate the network in other pieces than the encoder did: tested).  They are
    fp32-roundoff close to, not bit-identical with, a CPU / hipBLASLt evaluation (different summation order):
    strings written here are decoded here.  ``precision="fp16"`` (opt-in, round 3's path) runs the layers on the
    tower's fp16 MFMA GEMMs instead (``lla_gemm_f16_ex``); CPU tensors take torch's fp32 Linear.

    ``precision="ordered"`` (opt-in) gives every output a DEFINED value instead: ``acc = +0; for k ascending over the
    padded K: acc = fmaf(x[k], w[k], acc); y = acc + bias; relu`` in IEEE binary32 (the contract in
    ``csrc/gemm_f32_ordered.hip``).  CUDA tensors run ``lla_gemm_f32_ordered`` (a VALU kernel), CPU tensors
    ``lla_gemm_f32_ordered_host`` on the same padded operands ([Npad8][Kpad8] weights): the same bits, so the table rows
    a CPU derives are the GPU's and strings written on either are decoded on either."""

    def __init__(self, in_dim, out_dim, n_hid_layers=1, hid_dim=128, precision="fp32"):
        super().__init__()
        if precision not in ("fp32", "fp16", "ordered"):
            raise ValueError("precision must be 'fp32', 'fp16' or 'ordered'")
        self.precision = precision
        layers = [nn.Linear(in_dim, hid_dim), nn.Identity(), nn.ReLU(), nn.Identity()]
        for _ in range(1, n_hid_layers):
            layers += [nn.Linear(hid_dim, hid_dim), nn.Identity(), nn.ReLU(), nn.Identity()]
        layers += [nn.Linear(hid_dim, out_dim)]
        self.module = nn.Sequential(*layers)
        self._packed = None

    def __getstate__(self):   # (device copies of the weights are a cache)
        state = self.__dict__.copy()
        state["_packed"] = None
        return state

    def _pack(self, dev):
        """Padded device copies of the Linear layers, cached per device / parameter version: fp32 [Npad8][Kpad8]
        (fp16 [Npad128][Kpad64] for the opt-in fp16 path) weights + fp32 biases."""
        lin = [m for m in self.module if isinstance(m, nn.Linear)]
        key = (str(dev), self.precision) + tuple((m.weight._version, m.bias._version, m.weight.data_ptr()) for m in lin)
        if self._packed is None:
            self._packed = {}
        cached = self._packed.get(str(dev))     # (one entry per device: an ordered module on the GPU also decodes on the host)
        if cached is None or cached[0] != key:
            half = self.precision == "fp16"
            gn, gk, wt = (128, 64, torch.float16) if half else (8, 8, torch.float32)
            packs = []
            for m in lin:
                n, k = m.weight.shape
                npad, kpad = -(-n // gn) * gn, -(-k // gk) * gk
                w = torch.zeros((npad, kpad), dtype=wt, device=dev)
                w[:n, :k] = m.weight.detach().to(dev, wt)
                b = torch.zeros(npad, dtype=torch.float32, device=dev)
                b[:n] = m.bias.detach().to(dev, torch.float32)
                packs.append((w, b, n, k, npad, kpad))
            self._packed[str(dev)] = cached = (key, packs)
        return cached[1]

    def forward(self, X):
        shape = X.shape
        X2 = X.reshape(-1, shape[-1])
        if not X2.is_cuda and self.precision != "ordered":
            return self.module(X2.float()).reshape(*shape[:-1], -1)
        packs = self._pack(X2.device)
        at = torch.float16 if self.precision == "fp16" else torch.float32
        a = torch.zeros((X2.shape[0], packs[0][5]), dtype=at, device=X2.device)
        a[:, :packs[0][3]] = X2.to(at)
        out_dim = packs[-1][2]
        return self._layers(a, packs)[:, :out_dim].float().reshape(*shape[:-1], out_dim)

    def _layers(self, a, packs, bufs=None):
        """The Linear (+ ReLU) layers on a padded input ``a`` [rows, Kpad of the first layer] -> the last layer's padded
        output [rows, Npad].  ``bufs``: one [rows, Npad] tensor per layer to write into instead of allocating."""
        L, dev = _lib.lib(), a.device
        rows = a.shape[0]
        half = self.precision == "fp16"
        for i, (w, b, n, k, npad, kpad) in enumerate(packs):
            last = i == len(packs) - 1
            c = torch.empty((rows, npad), dtype=a.dtype, device=dev) if bufs is None else bufs[i]
            if self.precision == "ordered":
                args = (_lib.ptr(a), a.shape[1], _lib.ptr(w), kpad, _lib.ptr(b), _lib.ptr(c), npad, rows, npad, kpad,
                        0 if last else 1)
                if a.is_cuda:
                    _lib.check(L.lla_gemm_f32_ordered(*args, _lib.stream_ptr(dev)), "lla_gemm_f32_ordered")
                else:
                    _lib.check(L.lla_gemm_f32_ordered_host(*args), "lla_gemm_f32_ordered_host")
            elif half:
                rc = L.lla_gemm_f16_ex(_lib.ptr(a), a.shape[1], _lib.ptr(w), _lib.ptr(b), _lib.ptr(c), npad, None, 0,
                                       rows, npad, kpad, _lib.LLA_EPI_F16 if last else _lib.LLA_EPI_RELU_F16,
                                       _lib.stream_ptr(dev))
                _lib.check(rc, "lla_gemm_f16_ex")
            else:
                # (a's width is the previous layer's Npad: a multiple of 8 >= this layer's K, padding columns 0)
                rc = L.lla_gemm_f32(_lib.ptr(a), a.shape[1], _lib.ptr(w), kpad, _lib.ptr(b), _lib.ptr(c), npad,
                                    rows, npad, kpad, 0 if last else 1, _lib.stream_ptr(dev))
                _lib.check(rc, "lla_gemm_f32")
            a = c          # (Npad is a valid Kpad of the next layer; padding columns are 0: zero weights, zero bias)
        return a

    def padded_shapes(self, device):
        """-> (Kpad of the first layer, [Npad of every layer]) of the fp32 device path: what a caller of
        :meth:`forward_padded` sizes its buffers by."""
        packs = self._pack(torch.device(device))
        return packs[0][5], [p[4] for p in packs]

    def forward_padded(self, a, bufs=None):
        """``forward`` for a caller that already holds the input as the first GEMM wants it: ``a`` is a contiguous fp32
        device matrix [rows, Kpad] whose columns beyond the input width are zero (``padded_shapes``).  Nothing is copied:
        returns the last layer's padded output [rows, Npad] (the result is its leading ``out_dim`` columns, row stride
        Npad), written into ``bufs[-1]`` when ``bufs`` (one [rows, Npad_i] fp32 tensor per layer) is given.  The same GEMM
        calls as ``forward`` on the same values: the same bits."""
        if self.precision not in ("fp32", "ordered"):
            raise NotImplementedError("forward_padded runs the fp32 and the ordered MLP only")
        packs = self._pack(a.device)
        if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != packs[0][5] or not a.is_contiguous():
            raise ValueError(f"a must be a contiguous fp32 [rows, {packs[0][5]}] matrix")
        _lib.require_cuda(a, "a")
        if bufs is not None and [tuple(b.shape) for b in bufs] != [(a.shape[0], p[4]) for p in packs]:
            raise ValueError("bufs must hold one [rows, Npad] tensor per layer")
        return self._layers(a, packs, bufs)


class HRateHyperprior(HRateEstimator):
    """Scale-hyperprior coder twin (``lossyless/rates.py:572-756``), inference time.

    ``compress(z)`` -> ``[z_strings, side_z_strings]``: the side information ``side_encoder(z_in)``
    goes through the factorized ``EntropyBottleneck`` (HIP, one row per lane, table row = channel),
    its decoded value drives ``z_encoder`` -> (scales, means) -> ``build_indexes``, and ``z_in`` is
    coded by ``GaussianConditional`` with those per-element table rows (HIP,
    ``lla_rans_encode_indexed``).  ``get_indexes_means_hat`` reproduces the reference verbatim,
    including that it passes the *scales* as ``means`` (rates.py:694-696 overwrite ``means_hat``
    with ``atleast_ndim(scales_hat, 4)``), while ``forward_help`` -- like the reference's, :631-678 -- evaluates the
    likelihood with the predicted means.  The two MLPs run in fp32 (``mlp_precision="fp16"`` opts in to the fp16
    GEMMs: strings are then only decodable by a module with the same setting).

    ``coded_means``: which means the coder subtracts before rounding and adds back after decoding.  ``"scales"`` (the
    default) is the reference's behaviour above, bit for bit: what every reference container was written with.
    ``"predicted"`` departs from rates.py:689-696 on purpose and codes with the second half of ``z_encoder``'s output, the
    means the trained likelihood (rates.py:647-650) is centred at; it needs ``is_pred_mean=True``.  The table row of an
    element comes from its scale in both modes.  The mode is a constructor argument, not part of ``state_dict()`` (which
    keeps loading ``strict=True`` into the reference's module), and no string or container records it: strings written in
    one mode and read in the other -- like strings read with another state dict -- decode to wrong values without an
    error.

    ``mlp_precision="ordered"`` (opt-in; see :class:`MLP`) is such a constructor argument too -- not in ``state_dict()``,
    not recorded in any string or container, free to combine with ``coded_means``, and with the same warning: strings
    written in one ``mlp_precision`` and read in another decode to wrong values without an error.  It gives both MLPs an
    arithmetic a CPU reproduces bit for bit, so besides ``encode_device`` / ``decode_device`` / ``represent_device`` the
    module offers ``encode_host`` / ``decode_host`` / ``represent_host`` (same layouts, same bytes, same values, no GPU), and
    ``compress`` / ``decompress`` take them for CPU tensors.  With any other ``mlp_precision`` the host forms raise.
    """

    def __init__(self, z_dim, factor_dim=5, side_z_dim=None, is_pred_mean=True, mlp_precision="fp32",
                 coded_means="scales", **kwargs):
        from .entropy import GaussianConditional
        if coded_means not in ("scales", "predicted"):
            raise ValueError(f"coded_means must be 'scales' or 'predicted', got {coded_means!r}")
        if coded_means == "predicted" and not is_pred_mean:
            raise ValueError("coded_means='predicted' needs is_pred_mean=True: without it z_encoder predicts no means")
        super().__init__(z_dim, **kwargs)
        self.coded_means = coded_means
        if side_z_dim is None:
            side_z_dim = max(10, z_dim // factor_dim)
        self.side_z_dim = side_z_dim
        self.is_pred_mean = is_pred_mean
        self.entropy_bottleneck = EntropyBottleneck(side_z_dim, **self.kwargs_ent_bottleneck)
        self.gaussian_conditional = GaussianConditional(None)
        self.mlp_precision = mlp_precision
        self.side_encoder, self.z_encoder = self.get_encoders()

    def get_encoders(self):
        """rates.py:617-629."""
        kwargs_mlp = dict(n_hid_layers=2, hid_dim=max(self.z_dim, 256), precision=self.mlp_precision)
        side_encoder = MLP(self.z_dim, self.side_z_dim, **kwargs_mlp)
        z_encoder = MLP(self.side_z_dim, self.z_dim * (2 if self.is_pred_mean else 1), **kwargs_mlp)
        return side_encoder, z_encoder

    def _exp_scaling(self):
        """``mlp_precision="ordered"``, outside autograd: exp(scaling) is evaluated on the HOST in float64 wherever the
        module lives (as ``EntropyBottleneck.device_tables`` does for the factorized model), so the coder on the GPU and
        the one on a CPU hold the same fp32 factors.  Cached per parameter version: no copy per call."""
        if self.mlp_precision != "ordered" or torch.is_grad_enabled():
            return super()._exp_scaling()
        key = (self.scaling.device, self.scaling._version, self.scaling.data_ptr())
        cached = getattr(self, "_host_exp", None)
        if cached is None or cached[0] != key:
            es = torch.exp(self.scaling.detach().to("cpu", torch.float64)).float().to(self.scaling.device)
            self._host_exp = cached = (key, es)
        return cached[1]

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        try:
            update_registered_buffers(self.gaussian_conditional, f"{prefix}gaussian_conditional",
                                      ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"],
                                      state_dict, policy="resize")
        except KeyError:
            pass
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward_help(self, z, _, __=None):
        """rates.py:631-678 (eval mode) -> ``(z_hat, -log q(z, s) per example, logs, other)`` with logs
        ``H_q_ZlS``, ``H_q_Z`` (= H_q_ZS, the reference's naming), ``H_q_S``, ``H_ZlX`` (+ the real rate's)."""
        nats_to_bits = 1.0 / math.log(BASE_LOG)

        def code_length(likelihood):           # -log q, summed over the latent dimension: [batch]
            return torch.log(likelihood).sum(-1).neg()

        z_in = self.process_z_in(z)
        # hyper-latent s through the factorized bottleneck, then the conditional model of z given s-hat
        s_hat, q_s = self.entropy_bottleneck(self.side_encoder(z_in))
        scales_hat, means_hat = self.chunk_params(self.z_encoder(s_hat))
        z_hat, q_z_given_s = self.gaussian_conditional(z_in, scales_hat, means=means_hat)
        len_s, len_z_given_s = code_length(q_s), code_length(q_z_given_s)
        len_joint = len_s + len_z_given_s
        # (the reference logs the joint length under the key H_q_Z, rates.py:660-661: kept, the evaluator reads it)
        logs = {"H_q_ZlS": len_z_given_s.mean() * nats_to_bits, "H_q_Z": len_joint.mean() * nats_to_bits,
                "H_q_S": len_s.mean() * nats_to_bits, "H_ZlX": 0}
        self._add_real_rate(z, logs)
        return self.process_z_out(z_hat), len_joint, logs, {}

    def chunk_params(self, gaussian_params):
        if self.is_pred_mean:
            scales_hat, means_hat = gaussian_params.chunk(2, -1)
        else:
            scales_hat, means_hat = gaussian_params, None
        return scales_hat, means_hat

    def _side_strings_to_rows(self, strings):
        """EntropyBottleneck.decompress of the lossyless wrapper (rates.py:68-71): [B, side_z_dim]."""
        return self.entropy_bottleneck.decompress(strings).reshape(len(strings), self.side_z_dim)

    def get_indexes_means_hat(self, side_z_strings):
        side_z_hat = self._side_strings_to_rows(side_z_strings)
        gaussian_params = self.z_encoder(side_z_hat)
        scales_hat, means_hat = self.chunk_params(gaussian_params)
        scales_hat = scales_hat.reshape(*scales_hat.shape, 1, 1)
        if self.coded_means == "predicted":
            means_hat = means_hat.reshape(*means_hat.shape, 1, 1)
        else:
            means_hat = scales_hat  # (sic) rates.py:695-696
        indexes = self.gaussian_conditional.build_indexes(scales_hat)
        return indexes, means_hat

    @torch.no_grad()
    def compress(self, z, parent=None):
        """rates.py:701-713 -> ``[z_strings, side_z_strings]``."""
        if not self.is_coder_updated:
            raise RuntimeError("call update() / prepare_compressor_() first")
        if self.mlp_precision == "ordered" and not z.is_cuda:
            payload, offsets = self.encode_host(z)
            off, blob = offsets.numpy(), payload.numpy().tobytes()
            rec = [blob[int(off[r]) + 4:int(off[r + 1])] for r in range(2 * z.shape[0])]
            return [rec[0::2], rec[1::2]]
        z_in = self.process_z_in(z)
        side_z = self.side_encoder(z_in)
        side_z_strings = self.entropy_bottleneck.compress(side_z.contiguous())
        indexes, means_hat = self.get_indexes_means_hat(side_z_strings)
        z_in = z_in.reshape(*z_in.shape, 1, 1)
        z_strings = self.gaussian_conditional.compress(z_in, indexes, means=means_hat)
        return [z_strings, side_z_strings]

    @torch.no_grad()
    def decompress(self, all_strings):
        """rates.py:715-724 -> z_hat [B, z_dim] fp32 on the GPU."""
        assert isinstance(all_strings, list) and len(all_strings) == 2
        z_strings, side_z_strings = all_strings
        if self.mlp_precision == "ordered" and self.scaling.device.type != "cuda":
            parts, off = [], [0]
            for pair in zip(z_strings, side_z_strings, strict=True):
                for s in pair:
                    parts += [len(s).to_bytes(4, "big"), bytes(s)]
                    off.append(off[-1] + 4 + len(s))
            payload = torch.frombuffer(bytearray(b"".join(parts) + b"\0\0\0\0"), dtype=torch.uint8)
            return self.decode_host(payload, torch.tensor(off, dtype=torch.int64), len(z_strings))
        indexes, means_hat = self.get_indexes_means_hat(side_z_strings)
        z_hat = self.gaussian_conditional.decompress(z_strings, indexes, means=means_hat)
        return self.process_z_out(z_hat.reshape(z_hat.shape[0], -1))

    # ---- device path: the same strings with nothing crossing the bus.  ``compress`` copies the side strings to the
    # host, re-joins and DECODES them to get s_hat back, builds the indexes in a 63-step torch loop and copies the z
    # strings out separately; here s_hat comes from the symbols the side encoder already produced (the coder is
    # lossless), and subtract / round / build_indexes / code are one kernel (``lla_gaussian_quantise_encode``).
    def _device_params(self):
        """What the fused kernels read besides the two models' coding tables, cached per parameter version: the affine
        as ``process_z_in`` evaluates it, the zero bias / unit scale the side path quantises with, the fp32 scale table."""
        gc = self.gaussian_conditional
        dev = self.scaling.device
        key = (dev, self.scaling._version, self.biasing._version, gc.scale_table.data_ptr(), gc.scale_bound.data_ptr())
        cached = getattr(self, "_dev_params", None)
        if cached is None or cached[0] != key:
            p = dict(bias=self.biasing.detach().float().contiguous(), exp_scale=self._exp_scaling().contiguous(),
                     side_bias=torch.zeros(self.side_z_dim, dtype=torch.float32, device=dev),
                     side_scale=torch.ones(self.side_z_dim, dtype=torch.float32, device=dev),
                     scale_table=gc.scale_table.detach().float().contiguous(),
                     scale_bound=float(gc.lower_bound_scale.bound.float().item()))
            self._dev_params = cached = (key, p)
        return cached[1]

    def _scales_of(self, side_sym):
        """Side symbols int32 [B, side_z_dim] -> (fp32 matrix the scales are the leading z_dim columns of, its row
        stride): ``z_encoder(sym + median)``, read in place by the kernels (``chunk_params`` would be a view too).  The
        predicted means are its next z_dim columns (``_means_ptr``)."""
        s_hat = side_sym.to(torch.float32) + self.entropy_bottleneck.device_tables()["median"][None, :]
        params = self.z_encoder(s_hat)
        if params.dtype != torch.float32 or params.stride(1) != 1:
            params = params.float().contiguous()
        return params, params.stride(0)

    def _means_ptr(self, params):
        """Address of the means inside the ``z_encoder`` output ``params`` (row stride: that of the scales), no copy."""
        return ctypes.c_void_p(params.data_ptr() + 4 * self.z_dim)

    def _check_device_path(self, what):
        if not self.is_coder_updated:
            raise RuntimeError("call update() / prepare_compressor_() first")
        _require_coder(self.entropy_bottleneck)
        _require_coder(self.gaussian_conditional)
        if self.scaling.device.type != "cuda":
            raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")

    @torch.no_grad()
    def encode_device(self, z, want_symbols=False):
        """z [B, z_dim] fp16 / fp32 on the GPU -> ``(payload, offsets)``: uint8 device tensor holding the interleaved
        length-prefixed records ``be32(len z_0) z_0 be32(len side_0) side_0 be32(len z_1) ...`` and int64 device tensor
        [2B+1] of record offsets (``offsets[-1]`` = bytes used).  Record 2i / 2i+1 are the bytes ``compress(z)`` returns
        as ``z_strings[i]`` / ``side_z_strings[i]``.  Nothing is copied to the host or synchronised.
        ``want_symbols``: also return ``dict(side_symbols, z_symbols, z_indexes)`` (int32 device tensors; tests)."""
        self._check_device_path("encode_device")
        if z.dim() != 2 or z.shape[1] != self.z_dim:
            raise ValueError(f"z must be [B, {self.z_dim}], got {tuple(z.shape)}")
        if z.dtype not in (torch.float16, torch.float32):
            z = z.float()
        z = z.contiguous()     # (the kernel reads dense rows: a strided view is copied)
        _lib.require_cuda(z, "z")
        L, dev, st = _lib.lib(), z.device, _lib.stream_ptr(z.device)
        B, C, S = z.shape[0], self.z_dim, self.side_z_dim
        p, ebt, gct = self._device_params(), self.entropy_bottleneck.device_tables(), self.gaussian_conditional.device_tables()

        def scratch_for(n):
            stride = int(L.lla_rans_max_encoded_bytes(n))
            return (stride, torch.empty(max(B, 1) * stride, dtype=torch.uint8, device=dev),
                    torch.empty(max(B, 1), dtype=torch.int32, device=dev))

        side_z = self.side_encoder(self.process_z_in(z)).contiguous()
        side_sym = torch.empty((B, S), dtype=torch.int32, device=dev)
        stride_s, scratch_s, len_s = scratch_for(S)
        rc = L.lla_quantise_encode(_lib.ptr(side_z), _lib.LLA_Z_F32, B, S, _lib.ptr(p["side_bias"]),
                                   _lib.ptr(p["side_scale"]), _lib.ptr(ebt["median"]), _lib.ptr(ebt["cdf"]), ebt["W"],
                                   _lib.ptr(ebt["cdf_len"]), _lib.ptr(ebt["offset"]), _lib.ptr(scratch_s), stride_s,
                                   _lib.ptr(len_s), _lib.ptr(side_sym), st)
        _lib.check(rc, "lla_quantise_encode")
        params, ld = self._scales_of(side_sym)
        z_sym = torch.empty((B, C), dtype=torch.int32, device=dev) if want_symbols else None
        z_idx = torch.empty((B, C), dtype=torch.int32, device=dev) if want_symbols else None
        stride_z, scratch_z, len_z = scratch_for(C)
        head = (_lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, B, C, _lib.ptr(p["bias"]),
                _lib.ptr(p["exp_scale"]), _lib.ptr(params), ld)
        tail = (_lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]), gct["T"], gct["W"],
                _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]), _lib.ptr(scratch_z), stride_z, _lib.ptr(len_z),
                _lib.ptr(z_sym), _lib.ptr(z_idx), st)
        if self.coded_means == "predicted":
            _lib.check(L.lla_gaussian_quantise_encode_means(*head, self._means_ptr(params), ld, *tail),
                       "lla_gaussian_quantise_encode_means")
        else:
            _lib.check(L.lla_gaussian_quantise_encode(*head, *tail), "lla_gaussian_quantise_encode")
        cap = max(B, 1) * (stride_z + stride_s + 8)
        payload = torch.empty(cap, dtype=torch.uint8, device=dev)
        offsets = torch.empty(2 * B + 1, dtype=torch.int64, device=dev)
        wsb = int(L.lla_rans_compact_pairs_workspace_bytes(B))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rc = L.lla_rans_compact_pairs(_lib.ptr(scratch_z), stride_z, _lib.ptr(len_z), _lib.ptr(scratch_s), stride_s,
                                      _lib.ptr(len_s), B, _lib.ptr(payload), cap, _lib.ptr(offsets), _lib.ptr(ws), wsb, st)
        _lib.check(rc, "lla_rans_compact_pairs")
        if want_symbols:
            return payload, offsets, dict(side_symbols=side_sym, z_symbols=z_sym, z_indexes=z_idx)
        return payload, offsets

    @torch.no_grad()
    def decode_device(self, payload, offsets, B):
        """Inverse of ``encode_device``: payload uint8 (at least 4 bytes longer than ``offsets[-1]``: the decoders read
        whole words) / offsets int64 [2B+1] on the GPU -> z_hat [B, z_dim] fp32 on the GPU, the values ``decompress``
        gives for the same strings.  The side records are decoded (``lla_rans_decode_batch_strided``), ``z_encoder``
        runs, then ``lla_gaussian_decode_dequantise`` (``lla_gaussian_decode_dequantise_means`` when
        ``coded_means="predicted"``).  ValueError if a record is malformed: the
        kernels bound every read and a damaged record sets its image's status, which costs ONE host sync per call, at the
        end, to read the statuses back."""
        self._check_device_path("decode_device")
        if offsets.dtype != torch.int64 or offsets.numel() != 2 * B + 1:
            raise ValueError("offsets must be int64 [2B+1]")
        if payload.dtype != torch.uint8 or payload.dim() != 1:
            raise ValueError("payload must be a 1-D uint8 tensor")
        payload, offsets = payload.contiguous(), offsets.contiguous()
        _lib.require_cuda(payload, "payload")
        _lib.require_cuda(offsets, "offsets")
        L, dev, st = _lib.lib(), payload.device, _lib.stream_ptr(payload.device)
        C, S = self.z_dim, self.side_z_dim
        p, ebt, gct = self._device_params(), self.entropy_bottleneck.device_tables(), self.gaussian_conditional.device_tables()
        side_sym = torch.empty((B, S), dtype=torch.int32, device=dev)
        status = torch.zeros((2, max(B, 1)), dtype=torch.int32, device=dev)
        rc = L.lla_rans_decode_batch_strided(_lib.ptr(payload), _lib.ptr(offsets), 1, 1, 2, B, S, _lib.ptr(ebt["cdf"]),
                                             ebt["W"], _lib.ptr(ebt["cdf_len"]), _lib.ptr(ebt["offset"]),
                                             _lib.ptr(side_sym), _lib.ptr(status[0]), st)
        _lib.check(rc, "lla_rans_decode_batch_strided")
        params, ld = self._scales_of(side_sym)
        z_hat = torch.empty((B, C), dtype=torch.float32, device=dev)
        head = (_lib.ptr(payload), _lib.ptr(offsets), 1, 0, 2, B, C, _lib.ptr(p["bias"]), _lib.ptr(p["exp_scale"]),
                _lib.ptr(params), ld)
        tail = (_lib.ptr(p["scale_table"]), p["scale_bound"], _lib.ptr(gct["cdf"]), gct["T"], gct["W"],
                _lib.ptr(gct["cdf_len"]), _lib.ptr(gct["offset"]), _lib.ptr(z_hat), _lib.ptr(status[1]), st)
        if self.coded_means == "predicted":
            _lib.check(L.lla_gaussian_decode_dequantise_means(*head, self._means_ptr(params), ld, *tail),
                       "lla_gaussian_decode_dequantise_means")
        else:
            _lib.check(L.lla_gaussian_decode_dequantise(*head, *tail), "lla_gaussian_decode_dequantise")
        if B and int(status.max()) != 0:
            raise ValueError("malformed rANS stream")
        return z_hat

    @torch.no_grad()
    def represent_device(self, z):
        """z -> the z_hat that ``decode_device(*encode_device(z))`` gives, without coding (the same fp32 operations in the
        same order: round(side - median) + median, z_encoder, round(z_in - means) + means, process_z_out; the means are
        the scales unless ``coded_means="predicted"``)."""
        self._check_device_path("represent_device")
        z_in = self.process_z_in(z)
        med = self.entropy_bottleneck.device_tables()["median"][None, :]
        s_hat = torch.round(self.side_encoder(z_in) - med) + med
        first = self.z_dim if self.coded_means == "predicted" else 0
        means = self.z_encoder(s_hat)[:, first:first + self.z_dim]
        return self.process_z_out(torch.round(z_in - means) + means)

    # ---- host path (``mlp_precision="ordered"`` only): the device path's steps on CPU tensors with the library's host
    # entry points -- the two MLPs on ``lla_gemm_f32_ordered_host`` (the device kernel's chain, bit for bit), the side
    # records on the factorized host coder, the z records on the host twins of the conditional kernels.  Same layout, same
    # bytes, same values as ``encode_device`` / ``decode_device`` / ``represent_device``; the module may live on either
    # device (a compressor on the GPU decodes a container on the host with CPU copies of its tables and weights).
    def _check_host_path(self, what):
        if self.mlp_precision != "ordered":
            raise NotImplementedError(
                f'{what} needs mlp_precision="ordered" (this module runs {self.mlp_precision!r}): the table rows come '
                "from z_encoder, and only the ordered MLP has an arithmetic a CPU reproduces bit for bit")
        if not self.is_coder_updated:
            raise RuntimeError("call update() / prepare_compressor_() first")
        _require_coder(self.entropy_bottleneck)
        _require_coder(self.gaussian_conditional)

    def _host_params(self):
        """CPU copies (contiguous numpy) of what ``_device_params`` and the two ``device_tables`` hold, cached like them."""
        import numpy as np
        p, ebt, gct = self._device_params(), self.entropy_bottleneck.device_tables(), self.gaussian_conditional.device_tables()
        key = (id(p), id(ebt), id(gct))
        cached = getattr(self, "_host_cache", None)
        if cached is None or cached[0] != key:
            host = lambda v: np.ascontiguousarray(v.detach().cpu().numpy()) if hasattr(v, "cpu") else v
            h = dict(bias=host(p["bias"]), exp_scale=host(p["exp_scale"]), scale_table=host(p["scale_table"]),
                     scale_bound=p["scale_bound"], eb={k: host(v) for k, v in ebt.items()},
                     gc={k: host(v) for k, v in gct.items()})
            self._host_cache = cached = (key, h, (p, ebt, gct))     # (the dicts are kept alive: their ids are the key)
        return cached[1]

    @staticmethod
    def _host_z(z, C):
        if z.dim() != 2 or z.shape[1] != C:
            raise ValueError(f"z must be [B, {C}], got {tuple(z.shape)}")
        if z.is_cuda:
            raise RuntimeError("the host path takes CPU tensors (encode_device / represent_device take the GPU's)")
        if z.dtype not in (torch.float16, torch.float32):
            z = z.float()
        return z.contiguous()

    def _host_side(self, z, h):
        """-> (z_in, side symbols int32 [B, S]) as ``encode_device`` derives them."""
        z_in = (z.float() + torch.from_numpy(h["bias"])) * torch.from_numpy(h["exp_scale"])
        side_z = self.side_encoder(z_in)
        return z_in, torch.round(side_z - torch.from_numpy(h["eb"]["median"])[None, :]).to(torch.int32)

    def _host_scales(self, side_sym, h):
        """``_scales_of`` on the host: (z_encoder output fp32 [B, C or 2C] contiguous, scales / means pointers, pitch)."""
        s_hat = side_sym.to(torch.float32) + torch.from_numpy(h["eb"]["median"])[None, :]
        params = self.z_encoder(s_hat).float().contiguous()
        means = ctypes.c_void_p(params.data_ptr() + 4 * self.z_dim) if self.coded_means == "predicted" else None
        return params, means, params.stride(0)

    @torch.no_grad()
    def encode_host(self, z, want_symbols=False):
        """``encode_device`` for a CPU tensor z [B, z_dim] fp16 / fp32, without a GPU: -> ``(payload, offsets)`` CPU tensors
        in the same layout (uint8 interleaved length-prefixed records + 4 spare bytes, int64 [2B+1]), the same bytes.
        ``want_symbols``: also ``dict(side_symbols, z_symbols, z_indexes)`` (int32 CPU tensors)."""
        import numpy as np
        self._check_host_path("encode_host")
        z = self._host_z(z, self.z_dim)
        h, L = self._host_params(), _lib.lib()
        B, C, S = z.shape[0], self.z_dim, self.side_z_dim
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _, side_sym = self._host_side(z, h)
        params, means, ld = self._host_scales(side_sym, h)
        z_sym = torch.empty((B, C), dtype=torch.int32) if want_symbols else None
        z_idx = torch.empty((B, C), dtype=torch.int32) if want_symbols else None
        eb, gc = h["eb"], h["gc"]

        def records(call, what):      # size, then write (LLA_ECAP reports the size needed)
            off = np.zeros(B + 1, dtype=np.uint64)
            rc = call(None, 0, P(off))
            if rc not in (_lib.LLA_OK, _lib.LLA_ECAP):
                _lib.check(rc, what)
            out = np.empty(max(int(off[-1]), 1), dtype=np.uint8)
            _lib.check(call(P(out), out.size, P(off)), what)
            return out.tobytes(), off

        side_sym_np = np.ascontiguousarray(side_sym.numpy())
        side, soff = records(lambda out, cap, off: L.lla_rans_encode_batch_host(
            P(side_sym_np), B, S, P(eb["cdf"]), eb["W"], P(eb["cdf_len"]), P(eb["offset"]), 1, out, cap, off),
            "lla_rans_encode_batch_host")
        zrec, zoff = records(lambda out, cap, off: L.lla_gaussian_quantise_encode_host(
            _lib.ptr(z), _lib.LLA_Z_F16 if z.dtype == torch.float16 else _lib.LLA_Z_F32, B, C, P(h["bias"]),
            P(h["exp_scale"]), _lib.ptr(params), ld, means, ld, P(h["scale_table"]), h["scale_bound"], P(gc["cdf"]),
            gc["T"], gc["W"], P(gc["cdf_len"]), P(gc["offset"]), 1, out, cap, off, _lib.ptr(z_sym), _lib.ptr(z_idx)),
            "lla_gaussian_quantise_encode_host")
        parts, offsets = [], np.zeros(2 * B + 1, dtype=np.int64)
        for i in range(B):
            parts += [zrec[int(zoff[i]):int(zoff[i + 1])], side[int(soff[i]):int(soff[i + 1])]]
            offsets[2 * i + 1] = offsets[2 * i] + len(parts[-2])
            offsets[2 * i + 2] = offsets[2 * i + 1] + len(parts[-1])
        payload = torch.frombuffer(bytearray(b"".join(parts) + b"\0\0\0\0"), dtype=torch.uint8)
        if want_symbols:
            return payload, torch.from_numpy(offsets), dict(side_symbols=side_sym, z_symbols=z_sym, z_indexes=z_idx)
        return payload, torch.from_numpy(offsets)

    @torch.no_grad()
    def decode_host(self, payload, offsets, B):
        """``decode_device`` without a GPU: payload uint8 / offsets int64 [2B+1] CPU tensors (what ``encode_host`` returns,
        or ``encode_device``'s copied to the host) -> z_hat [B, z_dim] fp32 CPU tensor, the same bits.  ValueError for
        offsets that leave the payload or a malformed record."""
        import numpy as np
        self._check_host_path("decode_host")
        if offsets.dtype != torch.int64 or offsets.numel() != 2 * B + 1:
            raise ValueError("offsets must be int64 [2B+1]")
        if payload.dtype != torch.uint8 or payload.dim() != 1:
            raise ValueError("payload must be a 1-D uint8 tensor")
        if payload.is_cuda or offsets.is_cuda:
            raise RuntimeError("decode_host takes CPU tensors (decode_device takes the GPU's)")
        body = np.ascontiguousarray(payload.numpy())
        off = np.ascontiguousarray(offsets.numpy())
        if B and (int(off[0]) < 0 or int(off[-1]) > body.size or bool((np.diff(off) < 0).any())):
            raise ValueError("malformed rANS stream")      # (the host coder reads where the offsets point)
        h, L = self._host_params(), _lib.lib()
        C, S = self.z_dim, self.side_z_dim
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        eb, gc = h["eb"], h["gc"]
        # the side records (odd ones), packed back to back for lla_rans_decode_batch_host
        blob = body.tobytes()
        side = [blob[int(off[2 * i + 1]):int(off[2 * i + 2])] for i in range(B)]
        soff = np.zeros(B + 1, dtype=np.uint64)
        np.cumsum(np.fromiter(map(len, side), dtype=np.uint64, count=B), out=soff[1:])
        side_body = np.frombuffer(b"".join(side) + b"\0\0\0\0", dtype=np.uint8)
        side_sym = np.zeros((B, S), dtype=np.int32)
        status = np.zeros((2, max(B, 1)), dtype=np.int32)
        _lib.check(L.lla_rans_decode_batch_host(P(side_body), P(soff), 1, B, S, P(eb["cdf"]), eb["W"], P(eb["cdf_len"]),
                                                P(eb["offset"]), P(side_sym), P(status[0])), "lla_rans_decode_batch_host")
        params, means, ld = self._host_scales(torch.from_numpy(side_sym), h)
        z_hat = torch.empty((B, C), dtype=torch.float32)
        off_u = off.astype(np.uint64)
        _lib.check(L.lla_gaussian_decode_dequantise_host(
            P(body), P(off_u), 1, 0, 2, B, C, P(h["bias"]), P(h["exp_scale"]), _lib.ptr(params), ld, means, ld,
            P(h["scale_table"]), h["scale_bound"], P(gc["cdf"]), gc["T"], gc["W"], P(gc["cdf_len"]), P(gc["offset"]),
            _lib.ptr(z_hat), P(status[1])), "lla_gaussian_decode_dequantise_host")
        if B and int(status.max()) != 0:
            raise ValueError("malformed rANS stream")
        return z_hat

    @torch.no_grad()
    def represent_host(self, z):
        """``represent_device`` for a CPU tensor: the z_hat that ``decode_host(*encode_host(z))`` gives, without coding."""
        self._check_host_path("represent_host")
        z = self._host_z(z, self.z_dim)
        h = self._host_params()
        z_in, side_sym = self._host_side(z, h)
        params, _, _ = self._host_scales(side_sym, h)
        first = self.z_dim if self.coded_means == "predicted" else 0
        means = params[:, first:first + self.z_dim]
        es, bias = torch.from_numpy(h["exp_scale"]), torch.from_numpy(h["bias"])
        return (torch.round(z_in - means) + means) / es - bias


def synthetic_hyperprior_state_dict(seed=0, z_dim=512):
    """Seeded random ``HRateHyperprior`` state dict with built coding tables, for tests and benchmarks (no hyperprior
    checkpoint ships with the reference; rates on these weights mean nothing).  A freshly initialised z_encoder predicts
    scales near zero, i.e. the first table row everywhere, so the scale half of its last layer gets a per-channel bias
    spread log-uniformly over (and past both ends of) the 64-level scale table -- 0.03 .. 400 against 0.11 .. 256 -- and
    larger weights, so that the row also varies from image to image; the side encoder's last layer is scaled up so that the
    side symbols are not all zero."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = HRateHyperprior(z_dim).eval()
        with torch.no_grad():
            m.scaling.normal_(0.3, 0.1)
            m.biasing.normal_(0, 0.1)
            m.side_encoder.module[-1].weight.mul_(8)
            last = m.z_encoder.module[-1]
            last.weight[:z_dim].mul_(8)
            spread = torch.exp(torch.linspace(math.log(0.03), math.log(400.0), z_dim))
            last.bias[:z_dim] = spread[torch.randperm(z_dim)]
        m.update(force=True)
        return {k: v.detach().clone() for k, v in m.state_dict().items()}
