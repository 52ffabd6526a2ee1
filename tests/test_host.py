"""CPU: the C-ABI library loads and exports what include/lossyless_amd.h declares, the
host entry points agree with the oracle, and the Python mirror of the reference interface
behaves like hub/compressor.py where no GPU is needed.  No device compute here."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import BETAS, GOLDEN, ROOT, load_tables
from lossyless_amd import _lib
from lossyless_amd import distributed as lla_dist
from lossyless_amd.entropy import EntropyBottleneck, pmf_to_quantized_cdf, update_registered_buffers
from oracle import cbind, container, eb


def test_library_exports_every_declared_symbol():
    with open(os.path.join(ROOT, "include", "lossyless_amd.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(lla_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(L, name), f"{name} declared in the header but not exported"
    assert declared == set(_lib.EXPORTS), "python binding and header disagree"
    assert _lib.lib().lla_abi_version() == _lib.ABI_VERSION == 4


def test_library_is_hip_for_gfx950():
    out = subprocess.run(["strings", "-a", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "lossyless_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), fn
    assert "oracle" not in open(os.path.join(ROOT, "hubconf.py")).read()


def test_pmf_to_quantized_cdf_matches_oracle():
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, 31, 32):
        for _ in range(50):
            p = rng.dirichlet(np.full(n, 0.3)).astype(np.float32)
            p[rng.random(n) < 0.2] *= 1e-7       # force empty bins / steals
            if p.sum() <= 0:
                continue
            try:
                want = cbind.pmf_to_quantized_cdf(p)
            except ValueError:                   # no donor frequency: both must refuse
                with pytest.raises(RuntimeError):
                    pmf_to_quantized_cdf(p)
                continue
            assert np.array_equal(pmf_to_quantized_cdf(p), want)


def test_pmf_to_quantized_cdf_error_codes():
    L = _lib.lib()
    out = np.zeros(4, np.uint32)
    bad = np.zeros(3, np.float32)
    rc = L.lla_pmf_to_quantized_cdf(bad.ctypes.data_as(ctypes.c_void_p), 3, 16,
                                    out.ctypes.data_as(ctypes.c_void_p))
    assert rc == -4  # LLA_EDATA: no mass
    assert L.lla_pmf_to_quantized_cdf(None, 3, 16, out.ctypes.data_as(ctypes.c_void_p)) == -1


def test_max_encoded_bytes_bounds_the_oracle_worst_case(tables_b005):
    C = 512
    worst = np.full(C, -2 ** 29, np.int32)  # every symbol escaped with an 8-digit payload
    s = cbind.rans_encode(worst, tables_b005["cdf"], tables_b005["cdf_len"], tables_b005["offset"])
    assert len(s) <= _lib.lib().lla_rans_max_encoded_bytes(C)


def test_container_index(tmp_path):
    strings = [b"abcd", b"", b"12345678", b"wxyz"]
    blob = np.frombuffer(container.container_bytes(strings), dtype=np.uint8).copy()
    L = _lib.lib()
    n = ctypes.c_uint32()
    off = np.zeros(5, np.uint64)
    rc = L.lla_container_index(blob.ctypes.data_as(ctypes.c_void_p), blob.size,
                               off.ctypes.data_as(ctypes.c_void_p), 5, ctypes.byref(n))
    assert rc == 0 and n.value == 4
    assert off.tolist() == [0, 8, 12, 24, 32]
    # truncated file -> LLA_EDATA ; small index -> LLA_ECAP
    assert L.lla_container_index(blob.ctypes.data_as(ctypes.c_void_p), blob.size - 1,
                                 off.ctypes.data_as(ctypes.c_void_p), 5, ctypes.byref(n)) == -4
    assert L.lla_container_index(blob.ctypes.data_as(ctypes.c_void_p), blob.size,
                                 off.ctypes.data_as(ctypes.c_void_p), 4, ctypes.byref(n)) == -2


@pytest.mark.parametrize("tag", BETAS)
def test_update_reproduces_frozen_tables(tag):
    """EntropyBottleneck.update() on the shipped parameters == the committed integer tables
    (derived per load in the reference, frozen here)."""
    sd = torch.load(os.path.join(ROOT, "lossyless_amd", "assets", f"beta{tag}_factorized_rate.pt"),
                    map_location="cpu", weights_only=True)
    m = EntropyBottleneck(512, init_scale=10, filters=[3, 3, 3, 3])
    update_registered_buffers(m, "entropy_bottleneck", ["_quantized_cdf", "_offset", "_cdf_length"], sd)
    m.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("entropy_bottleneck.")})
    tab = load_tables(tag)
    assert m.update() is False                      # tables came frozen with the state dict
    assert np.array_equal(m._quantized_cdf.numpy(), tab["cdf"])
    assert m.update(force=True) is True             # re-derive: fp32 torch-CPU + C-ABI A12
    diff = np.abs(m._quantized_cdf.numpy().astype(np.int64) - tab["cdf"])
    # same image => identical; another libm may move a handful of 16-bit edges (F6)
    assert (diff != 0).mean() < 0.02
    assert np.array_equal(m._cdf_length.numpy(), tab["cdf_len"])
    assert np.array_equal(m._offset.numpy(), tab["offset"])


@pytest.mark.parametrize("tag", BETAS)
def test_fp64_derivation_brackets_fp32_tables(tag):
    """Independent float64 evaluation of A11 stays within a few counts of the frozen tables."""
    sd = torch.load(os.path.join(ROOT, "lossyless_amd", "assets", f"beta{tag}_factorized_rate.pt"),
                    map_location="cpu", weights_only=True)
    t64 = eb.derive_tables(sd, "fp64")
    tab = load_tables(tag)
    assert np.array_equal(t64["cdf_len"], tab["cdf_len"]) and np.array_equal(t64["offset"], tab["offset"])
    d = np.abs(t64["cdf"].astype(np.int64) - tab["cdf"])
    assert d.max() <= 64 and (d != 0).mean() < 0.02
    assert np.array_equal(t64["exp_scale"], tab["exp_scale"])


def test_hub_factories_on_cpu_build_reference_shaped_module():
    import hubconf
    comp, transform = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    assert comp.z_dim == 512 and comp.device == "cpu" and not comp.training
    keys = set(comp.state_dict().keys())
    want = {"scaling", "biasing", "entropy_bottleneck.quantiles", "entropy_bottleneck.target",
            "entropy_bottleneck._offset", "entropy_bottleneck._quantized_cdf",
            "entropy_bottleneck._cdf_length", "entropy_bottleneck.likelihood_lower_bound.bound"}
    want |= {f"entropy_bottleneck._matrix{i}" for i in range(5)}
    want |= {f"entropy_bottleneck._bias{i}" for i in range(5)}
    want |= {f"entropy_bottleneck._factor{i}" for i in range(4)}
    assert keys == want                              # the reference's 22 entries
    tab = load_tables("5e-02")
    assert np.array_equal(comp.entropy_bottleneck._quantized_cdf.numpy(), tab["cdf"])
    # reference error convention: CPU compress_dataset raises ValueError (hub/compressor.py:180)
    with pytest.raises(ValueError):
        comp.compress_dataset(torch.zeros(1, 3, 224, 224), "/tmp/never.bin")
    # no CPU fallback for the compute path
    with pytest.raises(RuntimeError):
        comp(torch.zeros(1, 3, 224, 224))
    # transform: PIL image -> [3,224,224] CLIP-normalised
    from PIL import Image
    img = Image.fromarray((np.random.default_rng(0).random((96, 96, 3)) * 255).astype(np.uint8))
    x = transform(img)
    assert tuple(x.shape) == (3, 224, 224) and x.dtype == torch.float32


def test_reference_state_dict_with_empty_tables_also_loads():
    """The reference's own checkpoints carry EMPTY tables -> update() derives."""
    from lossyless_amd import ClipCompressor
    sd = torch.load(os.path.join(ROOT, "lossyless_amd", "assets", "beta5e-02_factorized_rate.pt"),
                    map_location="cpu", weights_only=True)
    for k in ("_quantized_cdf", "_offset", "_cdf_length"):
        sd["entropy_bottleneck." + k] = torch.IntTensor()
    comp = ClipCompressor(sd, device="cpu", clip_weights="synthetic")
    assert comp.entropy_bottleneck._quantized_cdf.shape == (512, 32)


def test_weight_blob_layout_roundtrip():
    from lossyless_amd.clip_vit import pack_weights, synthetic_vit_state_dict
    sd = synthetic_vit_state_dict(3)
    blob = pack_weights(sd)
    L = _lib.lib()
    off = L.lla_vit_b32_param_offset(_lib.VIT_LAYER["FC_W"], 7)
    got = blob[off:off + 3072 * 768 * 2].view(np.float16).reshape(3072, 768)
    assert np.array_equal(got, sd["transformer.resblocks.7.mlp.c_fc.weight"].half().numpy())
    off = L.lla_vit_b32_param_offset(_lib.VIT_GLOBAL["CONV1_NHWC"], 0)
    got = blob[off:off + 768 * 3072 * 2].view(np.float16).reshape(768, 32, 32, 3)
    assert np.array_equal(got, sd["conv1.weight"].permute(0, 2, 3, 1).half().numpy())
    off = L.lla_vit_b32_param_offset(_lib.VIT_GLOBAL["PROJ_T"], 0)
    got = blob[off:off + 512 * 768 * 2].view(np.float16).reshape(512, 768)
    assert np.array_equal(got, sd["proj"].t().half().numpy())
    assert L.lla_vit_b32_param_offset(99, 0) == ctypes.c_size_t(-1).value
    # offsets are disjoint and cover the blob
    spans = []
    for pid in _lib.VIT_GLOBAL.values():
        spans.append((L.lla_vit_b32_param_offset(pid, 0), L.lla_vit_b32_param_bytes(pid)))
    for l in range(12):
        for pid in _lib.VIT_LAYER.values():
            spans.append((L.lla_vit_b32_param_offset(pid, l), L.lla_vit_b32_param_bytes(pid)))
    spans.sort()
    for (a, n), (b, _) in zip(spans, spans[1:]):
        assert a + n <= b
    assert spans[-1][0] + spans[-1][1] <= L.lla_vit_b32_weights_bytes()


def test_container_helpers_have_reference_format(tmp_path):
    from lossyless_amd import compressor as C
    p = tmp_path / "x.bin"
    with open(p, "wb") as f:
        C.write_uints(f, (3,))
        C.write_uints(f, (4,))
        C.write_bytes(f, b"abcd")
        C.write_uints(f, (0,))
        C.write_bytes(f, b"")
    assert p.read_bytes() == struct.pack(">II", 3, 4) + b"abcd" + struct.pack(">I", 0)
    with open(p, "rb") as f:
        assert C.read_uints(f, 1) == (3,)
        assert C.read_bytes(f, C.read_uints(f, 1)[0]) == b"abcd"


def test_shard_bounds_partition_in_order():
    for n in (0, 1, 7, 8, 1000003):
        for w in (1, 2, 3, 8):
            b = [lla_dist.shard_bounds(n, r, w) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n
            assert all(x[1] == y[0] for x, y in zip(b, b[1:]))
            assert max(h - l for l, h in b) - min(h - l for l, h in b) <= 1


_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from lossyless_amd import distributed as D
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[2],
                        rank=int(sys.argv[3]), world_size=int(sys.argv[4]))
rank, world = D.rank_world()
n = int(sys.argv[5])
lo, hi = D.shard_bounds(n, rank, world)
# record i = be32(len) + i repeated (i+1) times, padded to 4 -> variable sizes per rank
recs = []
for i in range(lo, hi):
    body = bytes([i]) * (4 * (i + 1))
    recs.append(len(body).to_bytes(4, "big") + body)
body = np.frombuffer(b"".join(recs), dtype=np.uint8)
labels = np.arange(lo, hi, dtype=np.uint16)
# (odd ranks hand over a torch tensor -- what RecordStream.finish() returns on a sending rank -- even ranks numpy)
b, l, n_all = D.gather_to_rank0(torch.from_numpy(body.copy()) if rank % 2 else body, labels, hi - lo, "cpu")
if rank == 0:
    want = b"".join(len(bytes([i]) * (4 * (i + 1))).to_bytes(4, "big") + bytes([i]) * (4 * (i + 1))
                    for i in range(n))
    assert n_all == n and b.tobytes() == want and l.tolist() == list(range(n))
    print("RANK0_OK")
else:
    assert b is None and l is None and n_all == n
D.barrier()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("world,n", [(2, 11), (8, 37), (8, 5), (8, 0)])
def test_gloo_gather_reassembles_dataset_order(tmp_path, world, n):
    """world_size 2 and 8 on CPU (gloo): rank-order concatenation of shard records == dataset order, with ragged
    shards (37 = 5 x 5 + 3 x 4), EMPTY shards (5 images on 8 ranks) and an empty dataset; the pinning helper
    leaves every rank at least one CPU."""
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    port = str(29500 + (os.getpid() * 7 + world * 13 + n) % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, port, str(r), str(world), str(n)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "RANK0_OK" in outs[0]


def test_pin_host_threads_partitions_the_cpus():
    import os as _os
    before = _os.sched_getaffinity(0)
    threads = torch.get_num_threads()
    try:
        slices = []
        for r in range(4):
            _os.sched_setaffinity(0, before)
            got = lla_dist.pin_host_threads(r, 4, max_threads=3)
            slices.append(frozenset(_os.sched_getaffinity(0)))
            assert got["cpus"] == len(slices[-1]) >= 1 and 1 <= got["threads"] <= 3
        if len(before) >= 4:
            assert all(a.isdisjoint(b) for i, a in enumerate(slices) for b in slices[i + 1:])
    finally:
        _os.sched_setaffinity(0, before)
        torch.set_num_threads(threads)


def test_rn50_weight_layout_and_oracle_shapes():
    """RN50-CLIP tower: 55 convolutions in execution order, disjoint blob spans,
    BatchNorm folding, and the oracle's output shape / fp16-storage error budget."""
    from lossyless_amd import clip_rn50
    from oracle import rn50 as orn50
    L = _lib.lib()
    names = clip_rn50.conv_names()
    assert len(names) == L.lla_rn50_conv_count() == 55
    d = (ctypes.c_int64 * 8)()
    spans, inplanes = [], None
    for i in range(len(names)):
        assert L.lla_rn50_conv_desc(i, d) == 0
        cin, cout, k, stride, kpad, npad, w_off, b_off = (int(v) for v in d)
        assert kpad % 64 == 0 and kpad >= cin * k * k and npad % 128 == 0 and npad >= cout and k in (1, 3)
        spans += [(w_off, npad * kpad * 2), (b_off, npad * 4)]
    o = (ctypes.c_int64 * 7)()
    assert L.lla_rn50_attnpool_offsets(o) == 0
    spans += [(int(v), 1) for v in o]
    spans.sort()
    for (a, n), (b, _) in zip(spans, spans[1:]):
        assert a + n <= b
    assert spans[-1][0] < L.lla_rn50_weights_bytes()
    assert L.lla_rn50_conv_desc(55, d) == -1
    sd = clip_rn50.synthetic_rn50_state_dict(2)
    w, b = clip_rn50.fold_bn(sd, "layer2.0.conv2", "layer2.0.bn2")
    x = torch.randn(1, 128, 5, 5)
    y_ref = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, sd["layer2.0.conv2.weight"], padding=1),
                                           sd["layer2.0.bn2.running_mean"], sd["layer2.0.bn2.running_var"],
                                           sd["layer2.0.bn2.weight"], sd["layer2.0.bn2.bias"], False, 0.0, 1e-5)
    assert torch.allclose(torch.nn.functional.conv2d(x, w, b, padding=1), y_ref, atol=1e-4)
    blob = clip_rn50.pack_weights(sd)
    assert blob.dtype == np.uint8 and blob.size == L.lla_rn50_weights_bytes()
    z = orn50.rn50_forward(sd, torch.randn(1, 3, 224, 224))
    assert tuple(z.shape) == (1, 1024) and bool(torch.isfinite(z).all())


def test_fused_bottleneck_refuses_what_it_does_not_take():
    """`lla_rn50_bottleneck_f16` (csrc/bottleneck_fused.hip) checks its shape before it touches the device: every refusal below
    returns LLA_EINVAL on a box without a GPU (the tower then runs the three kernels, csrc/rn50.hip).  The kernel itself:
    tests/test_gpu_rn50.py."""
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint8)
    a = buf.ctypes.data_as(ctypes.c_void_p)
    b = ctypes.c_void_p(buf.ctypes.data + (1 << 40))                  # "far away": no overlap with a (never dereferenced)

    def call(x=a, n=1, H=56, W=56, pitch=256, cin=256, k1=256, k2=576, k3=64, out=b, ldo=256, w=a):
        return L.lla_rn50_bottleneck_f16(x, n, H, W, pitch, cin, w, k1, w, w, k2, w, w, k3, w, out, ldo, None)

    assert call(n=0) == 0                                              # nothing to do
    assert call(n=-1) == -1 and call(x=None) == -1 and call(w=None) == -1
    assert call(cin=128) == -1 and call(H=55) == -1 and call(W=15) == -1
    assert call(pitch=248) == -1 and call(pitch=260) == -1 and call(ldo=192) == -1
    assert call(k1=128) == -1 and call(k2=512) == -1 and call(cin=64, pitch=64, k1=64, k3=64) == -1   # first block: K = 128
    assert call(n=1400) == -1                                          # 32-bit byte offsets of the halo loads
    assert call(out=a) == -1                                           # in place: halos are read after neighbours are written


def test_clip_weight_loading_from_a_torchscript_archive_and_a_prefixed_dict(tmp_path):
    """hub/compressor.py:39-40 does ``clip.load("ViT-B/32", jit=False)`` and keeps ``model.visual``.  Offline the
    weights come from a file: the OpenAI download is a TorchScript archive whose state-dict keys carry the
    ``visual.`` prefix; a plain (prefixed or bare) state-dict file must work too.  A scripted dummy module with the
    real key names and shapes stands in for ViT-B-32.pt; all three routes must pack to the same blob."""
    from lossyless_amd import clip_vit

    sd = clip_vit.synthetic_vit_state_dict(7)

    class Node(torch.nn.Module):
        def forward(self):   # (never called: the archive is only a container of named tensors)
            return 0

    def tree(flat):
        root = Node()
        for key, value in flat.items():
            parts, node = key.split("."), root
            for p in parts[:-1]:
                if not hasattr(node, p):
                    node.add_module(p, Node())
                node = getattr(node, p)
            node.register_parameter(parts[-1], torch.nn.Parameter(value.half(), requires_grad=False))
        return root

    clip_model = Node()
    clip_model.add_module("visual", tree(sd))
    clip_model.register_parameter("logit_scale", torch.nn.Parameter(torch.ones([]), requires_grad=False))
    clip_model.add_module("transformer", tree({"resblocks.0.ln_1.weight": torch.ones(512)}))   # the TEXT tower: ignored
    archive = tmp_path / "ViT-B-32.pt"
    torch.jit.script(clip_model).save(str(archive))
    got = clip_vit.load_clip_visual_state_dict(str(archive))
    assert set(got) == set(sd) and all(tuple(got[k].shape) == tuple(sd[k].shape) for k in sd)
    want = clip_vit.pack_weights({k: v.half() for k, v in sd.items()})
    assert np.array_equal(clip_vit.pack_weights(got), want)
    # a plain dict with the prefix, and one inside {"state_dict": ...}
    prefixed = tmp_path / "prefixed.pt"
    torch.save({"visual." + k: v.half() for k, v in sd.items()} | {"logit_scale": torch.ones([])}, prefixed)
    assert np.array_equal(clip_vit.pack_weights(clip_vit.load_clip_visual_state_dict(str(prefixed))), want)
    nested = tmp_path / "nested.pt"
    torch.save({"state_dict": {k: v.half() for k, v in sd.items()}}, nested)
    assert np.array_equal(clip_vit.pack_weights(clip_vit.load_clip_visual_state_dict(str(nested))), want)
    # resolve_clip_weights takes the path from the environment, as hubconf does
    os.environ["LOSSYLESS_CLIP_WEIGHTS"] = str(archive)
    try:
        sd2, desc = clip_vit.resolve_clip_weights(None)
    finally:
        del os.environ["LOSSYLESS_CLIP_WEIGHTS"]
    assert desc == str(archive) and set(sd2) == set(sd)


def test_rn50_flop_count_matches_the_convolutions_the_oracle_executes(monkeypatch):
    """bench.py's RN50 roofline numerator (clip_rn50.rn50_macs_per_image) is exact: it equals the MACs of every
    F.conv2d the fp32 oracle tower executes on one image (counted from the actual weight / output shapes) plus the
    attention pool's projections and single-query attention."""
    import torch.nn.functional as F
    from lossyless_amd import clip_rn50
    from oracle import rn50 as orn50
    seen = []
    real = F.conv2d

    def counting(t, w, b=None, **kw):
        y = real(t, w, b, **kw)
        seen.append(int(y.shape[2] * y.shape[3] * w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3]))
        return y

    monkeypatch.setattr(orn50.F, "conv2d", counting)
    orn50.rn50_forward(clip_rn50.synthetic_rn50_state_dict(1), torch.randn(1, 3, 224, 224))
    total, stages = clip_rn50.rn50_macs_per_image()
    assert len(seen) == 55
    assert sum(seen) == total - stages["attnpool"]
    assert stages["attnpool"] == 2048 * 2048 + 50 * 2 * 2048 * 2048 + 2 * 50 * 2048 + 1024 * 2048
    assert abs(2 * total / 1e9 - 11.586) < 1e-3


def test_package_import_selects_gtt_pinned_memory_unless_the_user_chose():
    """lossyless_amd/__init__.py: HSA_USERPTR_FOR_PAGED_MEM=0 by default (fork()-safe pinned memory for the
    DataLoader workers of the reference call), never over an explicit setting."""
    import subprocess
    code = "import os, lossyless_amd; print(os.environ['HSA_USERPTR_FOR_PAGED_MEM'])"
    for given, want in ((None, "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "HSA_USERPTR_FOR_PAGED_MEM"}
        if given is not None:
            env["HSA_USERPTR_FOR_PAGED_MEM"] = given
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip() == want


def test_weight_blob_moves_in_pieces():
    """``_lib.upload_in_pieces``: the packed weights never cross as one pageable copy of >= 128 MB (the HIP runtime
    would pin the source in place and keep it registered, which stalls the GPU at every later fork())."""
    from lossyless_amd import _lib

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("blob", torch.arange(1000, dtype=torch.int16), persistent=False)

    m = M()
    # CPU -> CPU and dtype-changing moves are left to nn.Module
    _lib.upload_in_pieces(m, "blob", lambda t: t.to("cpu"))
    _lib.upload_in_pieces(m, "blob", lambda t: t.float())
    assert m.blob.dtype == torch.int16 and m.blob.device.type == "cpu"
    m2 = m.to("cpu")
    assert torch.equal(m2.blob, torch.arange(1000, dtype=torch.int16))


@pytest.mark.gpu
def test_weight_blob_upload_on_gpu_is_exact():
    from lossyless_amd.clip_vit import VisionTransformer, synthetic_vit_state_dict
    v = VisionTransformer(synthetic_vit_state_dict(1))
    host = v.blob.clone()
    v = v.to("cuda")
    assert v.blob.is_cuda and torch.equal(v.blob.cpu(), host)


class _FakeTower:   # what _lib.Tower looks like to pickle: an object holding a ctypes pointer
    def __init__(self):
        self.handle = ctypes.c_void_p(0x1234)
        self.device = torch.device("cpu")


def test_tower_modules_pickle_and_deepcopy_with_a_live_handle():
    """after a forward the tower modules hold a ctypes handle (``_lib.Tower``) and a device workspace;
    ``pickle`` / ``copy.deepcopy`` / ``torch.save`` of the compressor must drop both (a ctypes pointer does not
    pickle, and two owners of one ``lla_tower_create`` handle would destroy it twice)."""
    import copy
    import io
    import pickle
    import hubconf

    FakeTower = _FakeTower
    comp, _ = hubconf.clip_compressor_b005(device="cpu", clip_weights="synthetic")
    comp.clip._tower = FakeTower()
    comp.clip._ws = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        pickle.dumps(comp.clip._tower)                  # the hazard itself
    clone = pickle.loads(pickle.dumps(comp))
    assert clone.clip._tower is None and clone.clip._ws is None
    assert torch.equal(clone.clip.blob, comp.clip.blob)
    deep = copy.deepcopy(comp)
    assert deep.clip._tower is None and comp.clip._tower is not None    # the original keeps its handle
    buf = io.BytesIO()
    torch.save(comp, buf)
    from lossyless_amd.clip_rn50 import ModifiedResNet
    rn = ModifiedResNet.__new__(ModifiedResNet)
    torch.nn.Module.__init__(rn)
    rn._tower, rn._ws, rn.chunk = FakeTower(), torch.zeros(4), 256
    assert pickle.loads(pickle.dumps(rn))._tower is None


def test_library_carries_the_sha_of_the_sources_it_was_built_from(tmp_path):
    """VERDICT r5 #4a: the .so files are git-ignored and travel prebuilt; one built from other sources than the
    tree's must be refused (and rebuilt by tests/conftest.py::_built), not tested in place of the code."""
    want = _lib.tree_sha()
    assert re.fullmatch(r"[0-9a-f]{16}", want)
    assert _lib.built_sha() == want and _lib.stale() is None
    assert _lib.lib().lla_source_sha().decode() == want
    # a doctored copy (another sha in the marker) is reported stale without being loaded; a missing file too
    blob = open(_lib.LIB_PATH, "rb").read()
    other = tmp_path / "liblossyless_amd.so"
    other.write_bytes(blob.replace(b"LLA_SOURCE_SHA=" + want.encode(), b"LLA_SOURCE_SHA=" + b"0" * 16))
    assert "built from sources 0000000000000000" in _lib.stale(str(other))
    assert "missing" in _lib.stale(str(tmp_path / "nope.so"))
    # the sha follows the sources: any edit of a kernel file changes it
    import importlib.util
    spec = importlib.util.spec_from_file_location("s", os.path.join(ROOT, "lossyless_amd", "csrc", "source_sha.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import shutil
    csrc = tmp_path / "a" / "b" / "csrc"
    shutil.copytree(os.path.join(ROOT, "lossyless_amd", "csrc"), csrc, ignore=shutil.ignore_patterns("build"))
    os.makedirs(tmp_path / "a" / "include")
    shutil.copy(os.path.join(ROOT, "include", "lossyless_amd.h"), tmp_path / "a" / "include")
    os.rename(tmp_path / "a" / "include", tmp_path / "include")   # (csrc/../../include)
    os.rename(tmp_path / "a" / "b" / "csrc", tmp_path / "a" / "csrc")
    assert mod.source_sha(str(tmp_path / "a" / "csrc")) == want
    with open(tmp_path / "a" / "csrc" / "common.h", "a") as f:
        f.write("\n// edit\n")
    assert mod.source_sha(str(tmp_path / "a" / "csrc")) != want


def _fake_sysfs(root, gpus):
    """A sysfs tree as gpu_partition reads it: KFD node 0 = a CPU (no SIMDs), then one node per GPU in `gpus` =
    [(render minor, numa node, num_xcc, CUs)], two NUMA nodes of 8 CPUs each."""
    kfd = root / "class/kfd/kfd/topology/nodes"
    (kfd / "0").mkdir(parents=True)
    (kfd / "0" / "properties").write_text("cpu_cores_count 16\nsimd_count 0\n")
    for i, (minor, numa, xcc, cus) in enumerate(gpus):
        (kfd / str(i + 1)).mkdir()
        (kfd / str(i + 1) / "properties").write_text(
            f"cpu_cores_count 0\nsimd_count {4 * cus}\nsimd_per_cu 4\nnum_xcc {xcc}\ndrm_render_minor {minor}\nname gfx950\n")
        dev = root / f"class/drm/renderD{minor}/device"
        dev.mkdir(parents=True)
        (dev / "numa_node").write_text(f"{numa}\n")
    for k, cl in enumerate(("0-7", "8-15")):
        nd = root / f"devices/system/node/node{k}"
        nd.mkdir(parents=True)
        (nd / "cpulist").write_text(cl + "\n")


def test_host_pinning_follows_the_gpus_numa_node_from_sysfs(tmp_path, monkeypatch):
    """pin_host_threads reads the NUMA node of the rank's GPU from sysfs (KFD node -> render minor ->
    device/numa_node -> cpulist) instead of assuming GPU i hangs off CPU slice i, and falls back to the contiguous slice
    where sysfs does not say."""
    import os as _os
    from lossyless_amd import gpu_partition as gp
    for v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "HSA_CU_MASK"):
        monkeypatch.delenv(v, raising=False)
    # four GPUs: 0 and 3 on node 1, 1 and 2 on node 0 -- NOT the order of the slices
    _fake_sysfs(tmp_path, [(128, 1, 8, 256), (129, 0, 8, 256), (130, 0, 8, 256), (131, 1, 8, 256)])
    sysfs = str(tmp_path)
    assert [n["drm_render_minor"] for n in gp.kfd_gpu_nodes(sysfs)] == [128, 129, 130, 131]
    assert gp.visible_gpus_without_hip(sysfs) == 4
    assert gp.gpu_numa_cpus(0, sysfs) == (1, list(range(8, 16))) and gp.gpu_numa_cpus(2, sysfs) == (0, list(range(8)))
    assert gp.gpu_numa_cpus(7, sysfs) == (None, [])
    before, threads = _os.sched_getaffinity(0), torch.get_num_threads()
    calls = []
    monkeypatch.setattr(_os, "sched_getaffinity", lambda pid: set(range(16)))
    monkeypatch.setattr(_os, "sched_setaffinity", lambda pid, cpus: calls.append(sorted(cpus)))
    try:
        got = [lla_dist.pin_host_threads(r, 4, sysfs=sysfs) for r in range(4)]
        assert [g["numa_node"] for g in got] == [1, 0, 0, 1] and all(g["source"] == "sysfs" and g["cpus"] == 4 for g in got)
        assert calls == [[8, 9, 10, 11], [0, 1, 2, 3], [4, 5, 6, 7], [12, 13, 14, 15]]
        # a visible-devices list re-indexes the devices: rank 0 of 1 on GPU 2 -> node 0, all 8 CPUs
        monkeypatch.setenv("HIP_VISIBLE_DEVICES", "2")
        calls.clear()
        one = lla_dist.pin_host_threads(0, 1, sysfs=sysfs)
        assert one["numa_node"] == 0 and calls == [list(range(8))]
        monkeypatch.delenv("HIP_VISIBLE_DEVICES")
        # numa_node -1 (single socket) / no sysfs at all: the contiguous slices of round 3
        (tmp_path / "class/drm/renderD128/device/numa_node").write_text("-1\n")
        calls.clear()
        fb = lla_dist.pin_host_threads(0, 4, sysfs=sysfs)
        assert fb["source"] == "slice" and fb["numa_node"] is None and calls == [[0, 1, 2, 3]]
        calls.clear()
        fb = lla_dist.pin_host_threads(3, 4, sysfs=str(tmp_path / "nowhere"), n_gpus=4)
        assert fb["source"] == "slice" and calls == [[12, 13, 14, 15]]
    finally:
        monkeypatch.undo()
        _os.sched_setaffinity(0, before)
        torch.set_num_threads(threads)


def test_cu_mask_geometry_comes_from_the_kfd_topology(tmp_path, monkeypatch):
    """partition_shared_gpu no longer hard-codes the MI355X's 8 x 32 CUs: XCD count and CUs per XCD are read
    from the GPU's KFD node (here a 304-CU part: eighths of 38 CUs), 8 x 32 only where they cannot be read."""
    from lossyless_amd import gpu_partition as gp
    for v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "HSA_CU_MASK"):
        monkeypatch.delenv(v, raising=False)
    _fake_sysfs(tmp_path, [(128, 0, 8, 304)])
    m = gp.partition_shared_gpu(1, 2, sysfs=str(tmp_path))
    assert m == "0:" + ",".join(str(i) for i in range(152, 304))
    monkeypatch.delenv("HSA_CU_MASK")
    m = gp.partition_shared_gpu(7, 8, sysfs=str(tmp_path))
    assert m == "0:" + ",".join(str(i) for i in range(266, 304))
    monkeypatch.delenv("HSA_CU_MASK")
    assert gp.partition_shared_gpu(0, 1, sysfs=str(tmp_path)) is None            # one rank per GPU: no mask
    m = gp.partition_shared_gpu(0, 2, sysfs=str(tmp_path / "nowhere"), if_unknown=1)
    assert m == "0:" + ",".join(str(i) for i in range(128))                        # unreadable: the MI355X's 8 x 32
    monkeypatch.delenv("HSA_CU_MASK")


# ---- GEMM selection (csrc/gemm_plan.h through lla_gemm_plan): which kernel, which tile height, how many workgroups ----
_GK = dict(none=0, tile128=1, tile256=2, persist1=3, persist2=4, pp=5, q4=6, w8=7)   # enum GemmKernel
_F16, _QGELU, _RESID, _PATCH, _RELU, _ADDRELU, _LNX = 0, 1, 2, 3, 4, 5, 9               # epilogues
_PLAIN, _NHWC, _NCHW, _CONV3 = 0, 1, 2, 3                                             # operand modes


def _expected_plan(epi, amode, M, N, K, lda, ldc, chunk, cus):
    """The product's selection, restated from the table at the top of csrc/gemm_plan.h independently of its code:
    -> (status, kernel, tile rows, workgroups)."""
    cdiv = lambda a, b: -(-a // b)
    refuse = (-1, 0, 0, 0)

    def persistent(kernel, tiles_n, tall_allowed, balanced):
        cost = {rows: cdiv(cdiv(M, rows) * tiles_n, cus) * rows for rows in (256, 320)}     # rounds x rows
        rows = 320 if tall_allowed and cost[320] <= cost[256] else 256
        tiles = cdiv(M, rows) * tiles_n
        grid = min(tiles, cus)
        if balanced and tiles > cus:            # as few workgroups as the same number of rounds needs, whole XCDs
            grid = min(cus, cdiv(cdiv(tiles, cdiv(tiles, cus)), 8) * 8)
        return (0, kernel, rows, grid)

    if M <= 0:
        return (0, 0, 0, 0)
    if N % 128 or K % 64:
        return refuse
    if (epi, amode) not in [(e, _PLAIN) for e in (_F16, _QGELU, _RESID, _RELU, _ADDRELU, _LNX)] + [
            (_PATCH, _NHWC), (_PATCH, _NCHW), (_RELU, _CONV3)]:
        return refuse
    panel = 256 * lda * 2 < 2 ** 31 and 256 * K * 2 < 2 ** 31 and M * lda * 2 < 2 ** 32 and N * K * 2 < 2 ** 32
    wide3 = N % 256 == 0 and N >= 768
    four_wave = M % 256 == 0 and N % 256 == 0 and N <= 3072 and K >= 256 and lda >= K and lda % 8 == 0 and panel
    tiles4 = (M // 256) * (N // 256)
    if epi == _LNX:
        if not (four_wave and N == 768 and ldc == 768 and M * 768 < 2 ** 32):      # (32-bit element offsets into x)
            return refuse
        return (0, _GK["q4"], 256, 256) if cus == 256 and tiles4 > cus else persistent(_GK["q4"], N // 256, False, True)
    if chunk and (epi != _PATCH or chunk % 256 or M < 9000 or not wide3 or K < 256):
        return refuse
    if epi in (_RESID, _PATCH) and (M + M // 49 + 2) * ldc >= 2 ** 32:
        return refuse
    stored = ldc if ldc < N else N
    # the 256-column persistent kernels store 16 bytes per lane into an fp16 row: its pitch must keep them aligned
    lines = ldc % 8 == 0 or epi not in (_F16, _QGELU, _RELU, _ADDRELU)
    if epi in (_RELU, _ADDRELU):
        if amode == _PLAIN and M >= 9000 and N % 256 == 0 and stored == N:
            return persistent(_GK["persist2"], N // 256, True, False) if lines else refuse
        if M > 128 or amode == _CONV3:
            return (0, _GK["tile256"], 256, cdiv(M, 256) * (N // 128))
        return (0, _GK["tile128"], 128, cdiv(M, 128) * (N // 128))
    if M <= 128:
        return (0, _GK["tile128"], 128, N // 128)
    if M < 9000:
        return (0, _GK["tile256"], 256, cdiv(M, 256) * (N // 128))
    if epi in (_F16, _QGELU) and N % 256 == 0 and N <= 3072 and K >= 128 and lda >= K and lda % 8 == 0 and ldc >= N and \
            ldc % 8 == 0 and panel:
        return persistent(_GK["w8"], N // 256, False, True)
    if epi == _RESID and ldc == N and four_wave:
        return persistent(_GK["q4"], N // 256, False, True)
    if wide3 and K >= 256:
        return persistent(_GK["pp"], N // 256, not chunk, True) if lines else refuse
    if wide3:
        return persistent(_GK["persist2"], N // 256, True, False) if lines else refuse
    return persistent(_GK["persist1"], N // 128, False, False)


def _tower_gemm_shapes(B):
    """(epilogue, operand mode, M, N, K, lda, ldc) of every GEMM of the ViT-B/32 tower on a slice of B images (csrc/tower.hip)."""
    M, row = 50 * B, 50 * 768
    return [(_PATCH, _NHWC, 49 * B, 768, 3072, 0, 768), (_PATCH, _NCHW, 49 * B, 768, 3072, 0, 768),
            (_F16, _PLAIN, M, 2304, 768, 768, 2304), (_RESID, _PLAIN, M, 768, 768, 768, 768),             # QKV, out-proj
            (_QGELU, _PLAIN, M, 3072, 768, 768, 3072), (_RESID, _PLAIN, M, 768, 3072, 3072, 768),          # c_fc, c_proj
            (_LNX, _PLAIN, M, 768, 768, 768, 768), (_LNX, _PLAIN, M, 768, 3072, 3072, 768),                # ... with LayerNorm
            # the last block: K and V for every token, everything else for the class rows alone (strided in place)
            (_F16, _PLAIN, M, 1536, 768, 768, 2304), (_F16, _PLAIN, B, 768, 768, row, 3 * row),
            (_RESID, _PLAIN, B, 768, 768, row, row), (_QGELU, _PLAIN, B, 3072, 768, 768, 3072),
            (_RESID, _PLAIN, B, 768, 3072, 3072, row), (_F16, _PLAIN, B, 512, 768, 768, 512)]               # final projection


def _rn50_gemm_shapes(n):
    """... and of every 1x1 / 3x3 convolution of the RN50-CLIP tower behind its direct stem convolution, n images a chunk."""
    from lossyless_amd import clip_rn50
    L, d, out = _lib.lib(), (ctypes.c_int64 * 8)(), []
    res = {"conv2": 112, "conv3": 112}
    r = 56
    for s, nb in enumerate(clip_rn50.BLOCKS):
        for b in range(nb):
            o = r // (2 if s > 0 and b == 0 else 1)
            p = f"layer{s + 1}.{b}."
            res.update({p + "conv1": r, p + "conv2": r, p + "conv3": o, p + "downsample.1": o})
            r = o
    for i, (name, _) in enumerate(clip_rn50.conv_names()):
        if name == "conv1":
            continue
        assert L.lla_rn50_conv_desc(i, d) == 0
        cin, cout, k, stride, kpad, npad = [int(v) for v in d][:6]
        M, ldc = n * res[name] ** 2, (npad if cout == npad else cout)
        if k == 3:
            out.append((_RELU, _CONV3, M, npad, kpad, cin, ldc))
        else:
            out += [(e, _PLAIN, M, npad, kpad, kpad, ldc) for e in (_RELU, _ADDRELU, _F16)]
    return out


def _plan_cases():
    cases = [s + (0,) for B in (4, 128, 129, 180, 257, 640, 1024, 8704) for s in _tower_gemm_shapes(B)]
    cases += [s + (0,) for n in (32, 256) for s in _rn50_gemm_shapes(n)]
    ms = sorted({m + d for m in (128, 256, 9000, 9216, 12800, 51200, 435200) for d in (-1, 0, 1)} | {0, 1, 100, 5000})
    for M in ms:
        for N in (128, 256, 512, 768, 2304, 3072):
            for K in (64, 128, 192, 256, 768, 3072):
                cases += [(e, _PLAIN, M, N, K, K, N, 0) for e in (_F16, _QGELU, _RESID, _RELU, _ADDRELU)]
                cases += [(_PATCH, _NCHW, M, N, K, 0, N, 0), (_RELU, _CONV3, M, N, K, 64, N, 0), (_RELU, _PLAIN, M, N, K, K, 64, 0)]
    cases += [(_PATCH, _NHWC, 49 * B, 768, 3072, 0, 768, 256) for B in (256, 1024, 8704)]      # the image batch in pieces
    # an output pitch that is a multiple of 4 and not of 8, below and above the persistent kernels' threshold
    cases += [(e, _PLAIN, M, N, K, K, N + 4, 0) for M in (5000, 9001) for N in (256, 768) for K in (64, 256)
              for e in (_F16, _QGELU, _RESID, _RELU, _ADDRELU)]
    return cases


def _plan_answers(L, cases, cus_list=(256, 304, 64)):
    k, rows, grid = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    out = []
    for cus in cus_list:
        for c in cases:
            rc = L.lla_gemm_plan(*c, cus, ctypes.byref(k), ctypes.byref(rows), ctypes.byref(grid))
            out.append((rc, k.value, rows.value, grid.value))
    return out


def test_gemm_selection_table():
    """Which kernel the tower's GEMM shapes reach, on which tiles and grid -- on 256 CUs (MI355X), and on 304 and 64 so that the
    grid arithmetic is not only checked where it happens to be a no-op."""
    L, cases = _lib.lib(), _plan_cases()
    for cus in (256, 304, 64):
        got = _plan_answers(L, cases, (cus,))
        for c, g in zip(cases, got):
            assert g == _expected_plan(*c, cus), (c, cus, g, _expected_plan(*c, cus))
    # ... and spelled out for the flagship batch: 8704 images on 256 CUs
    at = lambda i: _plan_answers(L, [_tower_gemm_shapes(8704)[i] + (0,)], (256,))[0]
    assert at(0) == (0, _GK["pp"], 320, 256)                                    # patch embedding: 1333 x 3 tall tiles, 16 rounds
    assert at(2) == (0, _GK["w8"], 256, 256) and at(4) == (0, _GK["w8"], 256, 256)      # QKV, c_fc
    assert at(3) == (0, _GK["q4"], 256, 256) and at(5) == (0, _GK["q4"], 256, 256)      # out-proj, c_proj: 5100 tiles, 20 rounds
    assert at(9)[1] == _GK["tile256"] and at(13) == (0, _GK["tile256"], 256, 34 * 4)     # class rows only, final projection
    b1024 = _plan_answers(L, [s + (0,) for s in _tower_gemm_shapes(1024)], (256,))
    assert b1024[0] == (0, _GK["pp"], 320, 240)       # 157 x 3 = 471 tall tiles in 2 rounds: 236 -> 240 workgroups
    assert b1024[2] == (0, _GK["w8"], 256, 232) and b1024[3] == (0, _GK["q4"], 256, 200)    # 1800 tiles in 8 rounds of 225; 600 in 3
    assert b1024[6] == (0, _GK["q4"], 256, 256)       # LayerNorm in the epilogue: the triple walk's 8 x 32 workgroups


def test_gemm_selection_refusals():
    """What the launchers answer LLA_EINVAL to, through the plan."""
    L = _lib.lib()
    plan = lambda *c, cus=256: _plan_answers(L, [c], (cus,))[0]
    ok = (_F16, _PLAIN, 12800, 768, 768, 768, 768, 0)
    assert plan(*ok)[0] == 0 and plan(_F16, _PLAIN, 0, 768, 768, 768, 768, 0) == (0, 0, 0, 0)       # nothing to do
    assert plan(_F16, _PLAIN, 12800, 192, 768, 768, 192, 0)[0] == -1            # N % 128
    assert plan(_F16, _PLAIN, 12800, 768, 96, 96, 768, 0)[0] == -1              # K % 64
    assert plan(_PATCH, _PLAIN, 12800, 768, 3072, 3072, 768, 0)[0] == -1 and plan(7, _PLAIN, *ok[2:])[0] == -1   # no such pair
    assert plan(_ADDRELU, _CONV3, 12800, 128, 576, 64, 128, 0)[0] == -1
    # fp32 epilogues: 32-bit element offsets into C (rows + rows / 49 + 2) * ldc
    assert plan(_RESID, _PLAIN, 5_400_000, 768, 768, 768, 768, 0)[0] == 0 and plan(_RESID, _PLAIN, 5_500_000, 768, 768, 768, 768, 0)[0] == -1
    # the image batch in pieces: patch embedding of >= 9000 rows in pieces of whole 256 images on the ping-pong kernel's 256-row tiles
    pieces = lambda M, chunk, epi=_PATCH, amode=_NHWC, N=768, K=3072: plan(epi, amode, M, N, K, 0 if amode else K, N, chunk)
    assert pieces(49 * 1024, 256) == (0, _GK["pp"], 256, 200)                   # (196 x 3 = 588 tiles in 3 rounds of 196 -> 200)
    assert pieces(49 * 1024, 100)[0] == -1 and pieces(49 * 128, 256)[0] == -1 and pieces(49 * 1024, 256, N=512)[0] == -1
    assert pieces(49 * 1024, 256, K=128)[0] == -1 and pieces(50 * 1024, 256, epi=_F16, amode=_PLAIN)[0] == -1
    # the four-wave kernel with LayerNorm (the tower asks before it plans a slice): whole tiles, N = ldc = 768, and c_proj's
    # operand panels within 32-bit byte offsets of A's base -- 14 080 images are the first slice of whole tiles beyond them
    lnx = lambda B, ldc=768: plan(_LNX, _PLAIN, 50 * B, 768, 3072, 3072, ldc, 0)[0]
    assert lnx(8704) == 0 and lnx(13824) == 0 and lnx(14080) == -1 and lnx(1000) == -1 and lnx(8704, ldc=1536) == -1
    # ... through lla_gemm_resid_layernorm768 the kernel takes what the tower never asks of it: a single row tile, the
    # shortest K -- and then rows enough to leave the epilogue's 32-bit element offsets into x (21 845 row tiles are the last)
    lnx_k = lambda M, K, lda=None: plan(_LNX, _PLAIN, M, 768, K, lda or K, 768, 0)
    assert lnx_k(256, 256) == (0, _GK["q4"], 256, 3) and lnx_k(768, 768) == (0, _GK["q4"], 256, 9)
    assert lnx_k(21760, 256) == (0, _GK["q4"], 256, 255) and lnx_k(22016, 256) == (0, _GK["q4"], 256, 256)
    assert lnx_k(256, 192)[0] == -1 and lnx_k(256, 256, lda=260)[0] == -1 and lnx_k(256, 256, lda=264)[0] == 0
    assert lnx_k(256 * 21845, 256)[0] == 0 and lnx_k(256 * 21846, 256)[0] == -1
    # ... and what the eight- / four-wave kernels leave to the ping-pong kernel instead of refusing
    assert plan(_F16, _PLAIN, 12800, 3328, 768, 768, 3328, 0)[1] == _GK["pp"]                   # N > 3072
    assert plan(_RESID, _PLAIN, 12837, 768, 768, 768, 768, 0)[1] == _GK["pp"]                   # ragged M
    assert plan(_F16, _PLAIN, 1_000_000, 768, 3072, 3072, 768, 0)[1] == _GK["pp"]               # M lda 2 >= 2^32
    # fp16 rows of pitch 8 k + 4: not through the 16-byte stores of the 256-column persistent kernels' epilogues
    assert plan(_ADDRELU, _PLAIN, 9001, 256, 64, 128, 324, 0)[0] == -1 and plan(_ADDRELU, _PLAIN, 9001, 256, 64, 128, 320, 0)[1] == _GK["persist2"]
    assert plan(_F16, _PLAIN, 9001, 768, 256, 256, 772, 0)[0] == -1 and plan(_RESID, _PLAIN, 9001, 768, 256, 256, 772, 0)[1] == _GK["pp"]
    assert plan(_ADDRELU, _PLAIN, 8999, 256, 64, 128, 324, 0)[1] == _GK["tile256"] and plan(_F16, _PLAIN, 9001, 256, 64, 64, 260, 0)[1] == _GK["persist1"]
    assert L.lla_gemm_plan(*ok, 0, None, None, None) == -1


def test_resid_layernorm_door_decides_from_the_arguments_alone():
    """lla_gemm_resid_layernorm768 takes what the plan takes for epi 9, N = ldc = 768, and says LLA_EINVAL to the rest before any
    device call (there is no device here); its workspace is one 16-byte granule per row and column tile + 6 words per row tile."""
    L = _lib.lib()
    size = L.lla_gemm_resid_layernorm768_workspace_bytes
    assert [size(M) for M in (-256, 0, 255, 256, 257, 768, 43776)] == [0, 0, 0, 12312, 0, 3 * 12312, 171 * 12312]
    p = ctypes.c_void_p(1 << 20)        # (never dereferenced: every call below is refused)
    call = lambda M, K, lda, rev=0, x=p, ws=p: L.lla_gemm_resid_layernorm768(p, lda, p, None, x, p, p, p, M, K, 24000, rev, ws, None)
    for M, K, lda in [(0, 256, 256), (255, 256, 256), (-256, 256, 256), (256, 192, 192), (256, 288, 288), (256, 256, 248),
                      (256, 256, 260), (256 * 21846, 256, 256), (50 * 14080, 3072, 3072)]:
        assert call(M, K, lda) == -1, (M, K, lda)
        assert _plan_answers(L, [(_LNX, _PLAIN, M, 768, K, lda, 768, 0)], (256,))[0][0] == (0 if M <= 0 else -1)
    assert call(256, 256, 256, rev=2) == -1 and call(256, 256, 256, rev=-1) == -1
    assert call(256, 256, 256, x=ctypes.c_void_p((1 << 20) + 4)) == -1 and call(256, 256, 256, x=None) == -1
    assert call(256, 256, 256, ws=None) == -1 and call(256, 256, 256, ws=ctypes.c_void_p((1 << 20) + 8)) == -1


def _rn50_forward_gemms(n, fuse_ds=True, fused_block=True, direct=True):
    """(epilogue, operand mode, M, N, K, lda, ldc) of every GEMM that lla_rn50_forward launches for a slice of n images, in its
    order, with the pitches it passes (rn50_slices, csrc/rn50.hip, restated; the three switches are LLA_RN50_FUSE_DS,
    LLA_RN50_FUSED_BLOCK and LLA_RN50_DIRECT of the tools/ build, all on in the product).  The direct convolutions and the fused
    bottleneck kernel are no GEMMs and do not appear."""
    L, d = _lib.lib(), (ctypes.c_int64 * 8)()

    def desc(fn, i):
        assert fn(i, d) == 0
        return [int(v) for v in d][:6]

    convs = [desc(L.lla_rn50_conv_desc, i) for i in range(L.lla_rn50_conv_count())]      # cin, cout, ksize, stride, kpad, npad
    fused = [desc(L.lla_rn50_fused_desc, s) for s in range(4)]                           # cin, cout, planes, inplanes, kpad, npad
    opitch = lambda c: c[5] if c[1] % 128 == 0 else (c[1] + 31) // 32 * 32
    out = []

    def conv(c, H, pitch, epi):
        cin, cout, ksize, stride, kpad, npad = c
        ldo = opitch(c) if epi in (_RELU, _ADDRELU) else npad
        if ksize == 1:
            out.append((epi, _PLAIN, n * H * H, npad, kpad, pitch, ldo))
        elif stride == 1 and direct and H % 8 == 0 and ((cin == 32 and cout in (32, 64)) or (cin == 64 and cout == 64)):
            pass                                                                         # conv_direct.hip
        elif stride == 1 and (cin % 64 == 0 or cin == 32):
            out.append((_RELU, _CONV3, n * H * H, npad, kpad, pitch, ldo))               # implicit GEMM
        elif not (direct and stride == 2 and cin == 3):
            Ho = (H - 1) // stride + 1
            out.append((epi, _PLAIN, n * Ho * Ho, npad, kpad, kpad, ldo))                # im2col matrix

    ci = 3
    conv(convs[0], 224, 3, _RELU)
    conv(convs[1], 112, opitch(convs[0]), _RELU)
    block0_fused = fused_block and fuse_ds and direct
    fuse0 = fuse_ds and direct and not block0_fused
    if not direct:
        conv(convs[2], 112, opitch(convs[1]), _RELU)
    H, pitch = 56, 128 if fuse0 else opitch(convs[2])
    from lossyless_amd import clip_rn50
    for s, nb in enumerate(clip_rn50.BLOCKS):
        for b in range(nb):
            stride = 2 if s > 0 and b == 0 else 1
            c1, c2, c3 = convs[ci:ci + 3]
            ci += 3
            if s == 0 and b == 0 and block0_fused:
                ci += 1
                pitch = c3[5]
                continue
            if s == 0 and b > 0 and fused_block and pitch == c3[5]:
                continue
            conv(c1, H, pitch, _RELU)
            Ho = H // stride
            if b == 0 and fuse_ds and (s > 0 or fuse0):
                ci += 1
                if s > 0:
                    conv(c2, H, opitch(c1), _RELU)
                out.append((_RELU, _PLAIN, n * Ho * Ho, fused[s][5], fused[s][4], fused[s][0], c3[5]))
                H, pitch = Ho, c3[5]
                continue
            conv(c2, H, opitch(c1), _RELU)
            if b == 0:
                conv(convs[ci], Ho, pitch, _F16)
                ci += 1
            conv(c3, Ho, opitch(c2), _ADDRELU)
            H, pitch = Ho, c3[5]
    assert ci == len(convs) and (H, pitch) == (7, 2048)
    out += [(_F16, _PLAIN, 50 * n, 4096, 2048, 2048, 4096), (_F16, _PLAIN, n, 2048, 2048, 50 * 2048, 2048),      # K | V, query
            (_F16, _PLAIN, n, 1024, 2048, 2048, 1024)]                                                          # output projection
    return out


def test_every_gemm_path_of_the_rn50_tower_has_a_kernel_level_case():
    """Every (kernel, epilogue, tile rows) that the RN50 tower's GEMMs reach on 256 CUs at chunks of 4, 64 and 192 images -- the
    product's calls and those of its A/B switches -- is one that a kernel-level float64 test runs: a case of
    test_gpu_rn50_gemms.py (which asserts its kernel and tile rows itself) or of test_gpu_rn50.py's two GEMM tables.  A change of
    the selection that sends the tower somewhere no such test goes fails here.  (No GEMM is launched.)"""
    import test_gpu_rn50
    import test_gpu_rn50_gemms as new
    L = _lib.lib()
    plan = lambda epi, amode, M, N, K, lda, ldc: _plan_answers(L, [(epi, amode, M, N, K, lda, ldc, 0)], (256,))[0]
    covered = set()
    for name, (M, N, K, lda, ldc, ldr, coff, epi, kernel, rows) in new.CASES.items():
        assert plan(epi, _PLAIN, M, N, K, lda, ldc)[:3] == (0, kernel, rows), name
        covered.add((kernel, epi, rows))
    for test in (test_gpu_rn50.test_gemm_ex_strided_relu_and_add_relu, test_gpu_rn50.test_gemm_ex_narrow_output_pitch):
        table = [m for m in test.pytestmark if m.name == "parametrize"]
        assert len(table) == 1 and table[0].args[0] == "M,N,K,lda,ldc,epi"
        for M, N, K, lda, ldc, epi in table[0].args[1]:
            rc, kernel, rows, _ = plan(epi, _PLAIN, M, N, K, lda, ldc)
            assert rc == 0
            covered.add((kernel, epi, rows))
    reached = {}
    for n in (4, 64, 192):
        for switches in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            calls = _rn50_forward_gemms(n, *switches)
            if switches == (True, True, True):       # the 13 bottlenecks behind layer1: 3 GEMMs each; the attention pool's 3
                assert len(calls) == 3 * 13 + 3
            for epi, amode, M, N, K, lda, ldc in calls:
                rc, kernel, rows, _ = plan(epi, amode, M, N, K, lda, ldc)
                assert rc == 0, (n, switches, epi, amode, M, N, K, lda, ldc)
                if amode == _CONV3:                  # (test_implicit_conv3x3_relu_against_float64: always this kernel)
                    assert kernel == _GK["tile256"]
                else:
                    reached.setdefault((kernel, epi, rows), (n, switches, M, N, K, lda, ldc))
    missing = {t: reached[t] for t in reached if t not in covered}
    assert not missing, missing
    # what the product itself adds to the one-tile kernels at these chunks
    product = {plan(*c)[1:3] + (c[0],) for n in (4, 64, 192) for c in _rn50_forward_gemms(n) if c[1] == _PLAIN}
    assert {(_GK["persist2"], 256, _RELU), (_GK["persist2"], 320, _ADDRELU), (_GK["pp"], 320, _F16)} <= product


_PLAN_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_host
from lossyless_amd import _lib
assert _lib.LIB_PATH.endswith("_ablation.so")
print("PLAN=" + json.dumps(test_host._plan_answers(_lib.lib(), test_host._plan_cases())))
"""


def _tools_build_answers(tmp_path, **switches):
    from conftest import ABLATION_LIB
    script = tmp_path / "plan.py"
    script.write_text(_PLAN_CHILD)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LLA_")}
    r = subprocess.run([sys.executable, str(script), ROOT], env=dict(env, LLA_LIB=ABLATION_LIB, **switches),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import json
    return [tuple(a) for a in json.loads(r.stdout.split("PLAN=")[1])]


def test_tools_build_selects_what_the_product_selects(tmp_path):
    """Every A/B number takes its baseline arm from the tools/ build: with no switch set it must choose the product's kernel,
    tile height and grid for every shape (the bits cannot tell: every kernel gives the same).  Then a few switches."""
    from conftest import ABLATION_LIB
    if not os.path.exists(ABLATION_LIB) or _lib.stale(ABLATION_LIB):
        pytest.skip("the tools/ build is not built: make -C lossyless_amd/csrc ablation")
    cases = _plan_cases()
    product = _plan_answers(_lib.lib(), cases)
    assert _tools_build_answers(tmp_path) == product
    n = len(cases)
    qkv = cases.index(_tower_gemm_shapes(8704)[2] + (0,))              # at 256 CUs: the first third of the answers
    patch1024 = cases.index(_tower_gemm_shapes(1024)[0] + (0,))
    assert product[qkv] == (0, _GK["w8"], 256, 256) and product[patch1024] == (0, _GK["pp"], 320, 240)
    off = _tools_build_answers(tmp_path, LLA_GEMM_W8="0")
    assert off[qkv] == (0, _GK["q4"], 256, 256)                        # the round-5 selection: the four-wave kernel
    assert [a for a, p in zip(off, product) if p[1] != _GK["w8"]] == [p for p in product if p[1] != _GK["w8"]]
    pp_only = _tools_build_answers(tmp_path, LLA_GEMM_W8="0", LLA_GEMM_Q4="0")
    assert pp_only[qkv] == (0, _GK["pp"], 320, 256) and not any(a[1] in (_GK["w8"], _GK["q4"]) for a, c in zip(pp_only, cases * 3) if c[0] != _LNX)
    t128 = _tools_build_answers(tmp_path, LLA_GEMM_W8="0", LLA_GEMM_Q4="0", LLA_GEMM_TILE="128")
    assert t128[qkv] == (0, _GK["tile128"], 128, 3400 * 18)
    full = _tools_build_answers(tmp_path, LLA_GEMM_BALANCED="0")
    assert full[patch1024] == (0, _GK["pp"], 320, 256) and full[qkv] == product[qkv] and len(full) == 3 * n


def test_objects_that_carry_the_source_sha_follow_every_hashed_file():
    """`make` must not report a library up to date whose sha the tree no longer has -- host.o is recompiled when
    any file source_sha.py hashes changes, in the product and in the tools/ build.  Dry runs: nothing is touched or compiled."""
    csrc = os.path.join(ROOT, "lossyless_amd", "csrc")
    listed = subprocess.run([sys.executable, "source_sha.py", "--list"], cwd=csrc, capture_output=True, text=True).stdout.split()
    assert "ablation/gemm_select.hip" in listed and "gemm_plan.h" in listed and "../../include/lossyless_amd.h" in listed
    for fn in ("tower.hip", "gemm_plan.h", "ablation/gemm_select.hip", "ablation/ablation.h", "../../include/lossyless_amd.h"):
        for target in ([], ["ablation"]):
            r = subprocess.run(["make", "-C", csrc, "-n", "-W", fn, *target], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            compiles = [l for l in r.stdout.splitlines() if "LLA_SOURCE_SHA" in l and l.rstrip().endswith("host.cpp")]
            assert len(compiles) == 1 and "-o build/host.o" in compiles[0], (fn, target, r.stdout)
