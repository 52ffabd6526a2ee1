#!/usr/bin/env python
"""bench.py -- encode img/sec + bits/img of clip_compressor_b005 on synthetic 224x224x3
batches (BASELINE.json metric / configs[1]), one process per GPU.

A step = one pass of the hot path over one batch already resident in HBM: NHWC fp16
images -> CLIP ViT-B/32 tower (HIP/MFMA) -> quantise + rANS (HIP) -> compaction into the
reference's container records -> host, driven through the same `RecordStream` that
`compress_dataset` loops with: the pushed 1024-image batches are gathered into tower passes of 8704
images (1700 row tiles: the persistent GEMMs' rounds come out full on 256 CUs), the entropy stage runs once per
`--entropy-group` x 1024 images (default 16) on a second stream and at the end of the timed region, so all bytes of
all timed batches are produced inside it (`--entropy-group 1` codes every ~1024 images on their own; the
bytes are the same).  With N > 1 every rank encodes its own batches (image
parallel, weak scaling, no data-path collective) and one RCCL gather at the end of the
timed region concatenates the bitstream on rank 0.

The timed region is exactly --steps steps after --warmup steps.  Prints ONE JSON line on rank 0 (contract in the
task description); a plain run measures only what that line's headline (`value`, `ms_per_step`) needs.  `--full`
adds, after the timed region, what takes runs of its own:
  roofline      -- the dominant kernel class (the tower GEMMs -- gemm_w8_kernel for QKV / c_fc, gemm_q4_kernel for the residual layers; MFMA bound): algorithmic
                   FLOPs / HIP-event time measured over extra passes of the timed size on the launch
                   stream, against the dense fp16 MFMA peak
  cpu_baseline  -- the CPU oracle (PIL resize + fp32 torch-CPU tower + C rANS, BASELINE configs[0]
                   shape) timed on the host's cores on a bounded sample (rank 0, N = 1 only)
  verified      -- after the timed region, the records of the timed batch are compared with the CPU
                   oracle's coding of the same embeddings, and 32 embeddings with the fp32 CPU tower
  shipped_affine and the *_stage legs -- the checkpoint's own affine, the entropy stage, preprocessing, the
                   hyperprior coder, STL10-shaped inputs, the reference's call and the RN50 tower, each timed alone
`--dump-outputs DIR` writes the records of the last timed step as .npy files (dump_outputs).

`python bench.py --gpus N` starts its own N ranks (torch.distributed.run on 127.0.0.1); under a
launcher (RANK / WORLD_SIZE set) it is one of the ranks.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP16_TFLOPS = 2500.0   # dense MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
# vector-memory bytes of one 256-row tile through one layer's four large GEMMs (256 x 256 x 64 tiles: 64 KB of operands per K-tile;
# epilogues: 128 KB of fp16 out, or 256 + 256 + 128 KB for x read / x written / LayerNorm output): QKV 9 column tiles x
# (12 x 64 + 128) KB, c_fc 12 x (12 x 64 + 128), out-proj 3 x (12 x 64 + 640), c_proj 3 x (48 x 64 + 640)
VMEM_BYTES_PER_ROW_TILE_LAYER = 1024 * (9 * 896 + 12 * 896 + 3 * 1408 + 3 * 3712)
FLOP_PER_IMG = 8.8176e9     # SURVEY.md 9.4 (2 x 4 408 811 520 MAC)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _synth_u8(B, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8)


def _normalise(u8, device):
    import torch
    u8 = u8.to(device)
    mean = torch.tensor(CLIP_MEAN, device=device)
    std = torch.tensor(CLIP_STD, device=device)
    return ((u8.float() / 255 - mean) / std).half().contiguous()


def synth_batch(B, seed, device):
    """u8 ~ U{0..255} i.i.d. (seeded) -> CLIP-normalised fp16, NHWC."""
    return _normalise(_synth_u8(B, seed), device)


def synth_batches(specs, device):
    """[synth_batch(B, seed, device) for (B, seed) in specs], the same images: the host's random draws (~1 s per
    1024 images, one generator each) run on threads of their own, so that set-up does not grow with the batches."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(len(specs), 16))) as ex:
        u8 = list(ex.map(lambda s: _synth_u8(*s), specs))
    return [_normalise(u, device) for u in u8]


def cpu_baseline(batch=32, min_seconds=10.0, max_seconds=30.0):
    """CPU restatement of BASELINE.json configs[0] (the reference's own CPU-runnable case):
    STL10-shaped uint8 96x96x3 images -> the reference's transform per image (PIL bicubic resize
    to 224 + centre crop + ToTensor + Normalize, hub/compressor.py:155,186 with
    utils/data/images.py:383-411) -> fp32 torch-CPU tower -> C rANS, batches of 32 (oracle/)."""
    import numpy as np
    import torch
    from PIL import Image
    from lossyless_amd.clip_vit import synthetic_vit_state_dict
    from lossyless_amd.preprocess import ClipPreprocess
    from oracle import cbind, eb, vit
    tab = dict(np.load(os.path.join(ROOT, "tests", "golden", "tables_5e-02.npz")))
    sd = synthetic_vit_state_dict(1)
    sd = {k: v.half().float() for k, v in sd.items()}
    ncpu = os.cpu_count() or 1
    rng = np.random.default_rng(0)
    raw = [Image.fromarray(rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)) for _ in range(batch)]
    transform = ClipPreprocess()

    def one_batch(imgs):
        xb = torch.stack([transform(im) for im in imgs])           # PIL resize: 1 thread, as a
        with torch.no_grad():                                      # DataLoader worker would
            z = vit.vit_b32_forward(sd, xb, weights_rounded_to_fp16=False).numpy()
        sym = eb.symbols_of(z.astype(np.float16).astype(np.float32), tab)
        pay, off = cbind.rans_encode_batch(sym, tab["cdf"], tab["cdf_len"], tab["offset"])
        return int(off[-1]) + 4 * len(imgs)

    # torch-CPU does not scale to hundreds of threads on a 32-image batch: probe a few
    # thread counts on 8 images each and keep the fastest (reported as `cores`)
    best, cores = None, 1
    for t in sorted({min(ncpu, c) for c in (8, 16, 32, 64, 128)}):
        torch.set_num_threads(t)
        one_batch(raw[:4])
        t0 = time.time()
        one_batch(raw[:8])
        dt = time.time() - t0
        if best is None or dt < best:
            best, cores = dt, t
        if dt > 6:
            break
    torch.set_num_threads(cores)
    t0 = time.time()
    for im in raw:
        transform(im)
    resize_s = (time.time() - t0) / batch
    n, nbytes, t0 = 0, 0, time.time()
    while True:
        nbytes += one_batch(raw)
        n += batch
        el = time.time() - t0
        if el >= min_seconds or el >= max_seconds:
            break
    # Where the reference itself spends its encode time (SURVEY.md A13 "dominant in reference"):
    # compressai codes ONE image per Python iteration and re-marshals the whole [512, W] table to
    # Python lists for every image.  Emulated here around the oracle's C coder (labelled emulation:
    # compressai itself is not installed): lists in, one call per image, bytes out.
    sym = eb.symbols_of(np.zeros((64, 512), np.float32), tab)
    t1, k = time.time(), 0
    while time.time() - t1 < 2.0:
        for srow in sym:
            cdfs, lens, offs = tab["cdf"].tolist(), tab["cdf_len"].tolist(), tab["offset"].tolist()
            cbind.rans_encode(np.asarray(srow.tolist(), dtype=np.int32), np.asarray(cdfs, dtype=np.int32),
                              np.asarray(lens, dtype=np.int32), np.asarray(offs, dtype=np.int32))
            k += 1
    per_image_loop = k / (time.time() - t1)
    # (what each field is: DESIGN.md section 6, "the bench line")
    return dict(value=round(n / el, 2), unit="img/s", cores=cores, kind="port",
                pil_resize_ms_per_img=round(1e3 * resize_s, 3),
                reference_shaped_coder_img_per_sec=round(per_image_loop, 1),
                sample=f"{n} STL10-shaped 96x96 u8 images, batch {batch}, {el:.1f}s: PIL resize + fp32 tower + C rANS",
                host_threads=ncpu, bits_per_img=round(8 * nbytes / n, 2))


def symbol_mismatch_rates(z, z_ref):
    """Fraction of the 512 symbols per image on which two sets of embeddings (HIP tower / fp32 oracle tower)
    quantise differently, per shipped rate point: symbol = round_half_even((z + bias) * exp(scaling) - median)
    (hub/compressor.py:105-109 + EntropyModel.quantize).  SURVEY.md section 7: report next to the embedding error."""
    import numpy as np
    import torch
    import hubconf
    from oracle import eb
    out = {}
    for tag, beta in (("b01", 1e-1), ("b005", 5e-2), ("b001", 1e-2)):
        sd = hubconf._weights_for(beta)
        tab = dict(bias=sd["biasing"].float().numpy(),
                   exp_scale=torch.exp(sd["scaling"].double()).float().numpy(),
                   median=sd["entropy_bottleneck.quantiles"][:, 0, 1].float().contiguous().numpy())
        a, b = eb.symbols_of(z, tab), eb.symbols_of(z_ref, tab)
        out[tag] = dict(rate=round(float((a != b).mean()), 6), symbols=int(a.size),
                        images_with_a_mismatch=int((a != b).any(axis=1).sum()))
    return out


def oracle_pin():
    """What the checker itself is pinned against, stated in every line that says `verified`: the
    reference's arithmetic for this path lives in pip packages that are not installed here (compressai==1.1.5, clip:
    /root/reference/requirements/environment.yaml:98,105) and the reference holds no golden vectors, so oracle/ is a
    restatement read against the published sources -- `pinned` only where tools/verify_against_compressai.py can run."""
    import importlib.util
    have = [m for m in ("compressai", "clip") if importlib.util.find_spec(m) is not None]
    if len(have) == 2:
        return "compressai and clip importable: run tools/verify_against_compressai.py (tests/test_reference_pin.py)"
    return "unpinned (compressai/clip absent)" if not have else f"unpinned ({' / '.join(sorted({'compressai', 'clip'} - set(have)))} absent)"


def verify_first_batch(comp, x):
    """Checker, run AFTER the timed region (never inside it): the records the timed loop produces
    for its batch must equal what the CPU oracle codes from the same embeddings, and those
    embeddings (first 8 images) must sit within 1e-3 of the fp32 CPU tower.  -> dict for the JSON."""
    import numpy as np
    from lossyless_amd.clip_vit import synthetic_vit_state_dict
    from oracle import cbind, eb, vit
    st = comp.record_stream(1)
    st.push(x)
    body = st.finish().tobytes()
    z = comp.clip(x)
    t = comp._tables()
    tab = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in t.items()}
    sym = eb.symbols_of(z.float().cpu().numpy(), tab)
    pay, off = cbind.rans_encode_batch(sym, tab["cdf"], tab["cdf_len"], tab["offset"])
    pay = pay.tobytes()
    want = b"".join(int(off[i + 1] - off[i]).to_bytes(4, "big") + pay[int(off[i]):int(off[i + 1])]
                    for i in range(len(sym)))
    out = dict(records_equal_oracle=bool(body == want), images=int(x.shape[0]), oracle_pin=oracle_pin())
    if comp.clip_weights_desc == "synthetic-seed1":
        xs = x[:32]
        xs = xs.permute(0, 3, 1, 2) if xs.shape[-1] == 3 else xs
        z_ref = vit.vit_b32_forward(synthetic_vit_state_dict(1), xs.float().cpu()).numpy()
        zz = z[:32].float().cpu().numpy()
        rel = float((np.linalg.norm(zz - z_ref, axis=1) / np.linalg.norm(z_ref, axis=1)).max())
        out.update(embedding_rel_err_max=round(rel, 6), embedding_ok=bool(rel < 1e-3), embedding_images=32,
                   symbol_mismatch_rate=symbol_mismatch_rates(zz, z_ref))
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, body, n_images, world, batch):
    """--dump-outputs: what the timed loop handed its caller for the images of its last step on every rank -- their
    container records (4-byte big-endian length + rANS payload per image, in image order; ranks in rank order),
    the bytes of a compress_dataset file -- as float32: DIR/records.npy (the bytes) and DIR/record_bytes.npy (each
    record's length).  Beyond DUMP_LIMIT_BYTES the first records that fit are kept."""
    import struct
    import numpy as np
    body = np.ascontiguousarray(body, dtype=np.uint8)
    ends = np.empty(n_images, np.int64)
    pos = 0
    for i in range(n_images):
        pos += 4 + struct.unpack_from(">I", body, pos)[0]
        ends[i] = pos
    assert pos == body.size, f"{body.size} record bytes, {pos} parsed"
    per_rank = n_images // world
    last = np.concatenate([np.arange(r * per_rank + per_rank - batch, (r + 1) * per_rank) for r in range(world)])
    lengths = ends[last] - np.where(last > 0, ends[last - 1], 0)
    keep = int(np.searchsorted(np.cumsum(lengths) * 4 + 4 * np.arange(1, last.size + 1), DUMP_LIMIT_BYTES, "right"))
    last, lengths = last[:keep], lengths[:keep]
    records = np.concatenate([body[e - n:e] for e, n in zip(ends[last], lengths)])
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "records.npy"), records.astype(np.float32))
    np.save(os.path.join(dirname, "record_bytes.npy"), lengths.astype(np.float32))


def kernel_source_sha():
    """Tag of the kernel sources a committed counter profile belongs to: sha256 over csrc/*.{hip,h,cpp} + the
    C-ABI header (the GPU box has no .git, so a commit id cannot be checked there)."""
    from lossyless_amd import _lib
    return _lib.tree_sha()


def calibrate_affine_(comp, device, images=4096, batch=1024, seed0=1000, spread=1.0):
    """Refit the compressor's per-dimension affine (``scaling`` / ``biasing``, hub/compressor.py:46-47,105-109) to
    the SYNTHETIC tower, in place, so that z_in = (z + biasing) * exp(scaling) follows the shipped b005 pmf of every
    channel: same median + mean offset, `spread` x the pmf's standard deviation.  The integer tables (the learned
    pmf, what the coder reads) are untouched.  Why: the shipped affine was fitted to real CLIP features; with seed-1
    random tower weights almost every symbol escapes the coding window (4107 bits/img, 8 payload digits per
    symbol) -- a stress case, not the workload.  Real CLIP features on STL10 code at 1506.6 bits/img
    (notebooks/Hub.ipynb:253) against a model entropy of 1365.6; this lands in between.  Returns a description."""
    import numpy as np
    import torch
    t = comp._tables()
    cdf, ln, off = (t[k].cpu().numpy() for k in ("cdf", "cdf_len", "offset"))
    med = t["median"].cpu().numpy().astype(np.float64)
    C = cdf.shape[0]
    pm, ps = np.zeros(C), np.zeros(C)
    for c in range(C):
        n = int(ln[c])
        body = np.diff(cdf[c, :n]).astype(np.float64)[:n - 2]     # (the last bin is the escape symbol)
        w = body / body.sum()
        k = np.arange(n - 2) + off[c]
        pm[c] = (w * k).sum()
        ps[c] = np.sqrt((w * (k - pm[c]) ** 2).sum())
    zs = [comp.clip(xb).float() for xb in synth_batches(
        [(min(batch, images - i), seed0 + i // batch) for i in range(0, images, batch)], device)]
    z = torch.cat(zs).double().cpu().numpy()
    m, sd = z.mean(0), z.std(0)
    es = spread * ps / sd
    bias = (med + pm) / es - m
    with torch.no_grad():
        comp.scaling.copy_(torch.from_numpy(np.log(es)).float().to(comp.scaling.device))
        comp.biasing.copy_(torch.from_numpy(bias).float().to(comp.biasing.device))
    return f"b005 frozen tables; affine refit to the synthetic tower on {images} calibration images"


def device_identity(index):
    """(device index, name, PCI bus id, uuid) of a visible GPU, for the N > 1 line: proves N distinct devices."""
    import torch
    p = torch.cuda.get_device_properties(index)
    bus = None
    if all(hasattr(p, k) for k in ("pci_domain_id", "pci_bus_id", "pci_device_id")):
        bus = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
    return dict(device=index, name=p.name, pci_bus_id=bus, uuid=str(getattr(p, "uuid", "")) or None)


def respawn_under_torchrun(n):
    """`python bench.py --gpus N` (no launcher): start N ranks of this script under
    torch.distributed.run on this node and hand through rank 0's JSON line."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs on this host
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=68, help="timed 1024-image steps (68 = 8 tower passes of 8704 images)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=1024, help="images per step per GPU")
    ap.add_argument("--chunk", type=int, default=0, help="images per tower slice (0 = default)")
    ap.add_argument("--layout", choices=["nhwc", "nchw"], default="nhwc")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure and check what the headline does not need: roofline "
                         "passes, CPU baseline, shipped affine, oracle check, the other stages (each --no-* below "
                         "drops one of them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write the records of the last timed step to DIR/*.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl")
    ap.add_argument("--dataset-images", type=int, default=0,
                    help="instead of timed steps: compress_dataset over N lazily generated images "
                         "(BASELINE configs[3]), sharded over the ranks, file written by rank 0")
    ap.add_argument("--keep-file", default="",
                    help="with --dataset-images: keep the .bin rank 0 wrote at this path (tests inspect it)")
    ap.add_argument("--entropy-group", type=int, default=16,
                    help="tower batches entropy-coded per launch sequence (1 = code every batch)")
    ap.add_argument("--host-images", type=int, default=0,
                    help="instead of timed steps: compress_dataset over N fp16 NHWC images held in "
                         "pinned HOST memory (the PCIe-inclusive rate; not the headline metric)")
    ap.add_argument("--no-extra", action="store_true",
                    help="skip the entropy-stage / preprocess legs (cleaner kernel traces)")
    ap.add_argument("--no-verify", action="store_true",
                    help="skip the post-timing check of the batch's records against the CPU oracle")
    ap.add_argument("--shipped-affine", action="store_true",
                    help="keep the shipped b005 scaling / biasing (fitted to real CLIP features): with the synthetic "
                         "tower nearly every symbol escapes -- the stress case, 4107 bits/img")
    ap.add_argument("--min-seconds", type=float, default=0.0,
                    help="the timed region repeats the block of --steps steps until it has run this long AND ends on "
                         "a whole tower pass (0, the default: exactly --steps steps)")
    ap.add_argument("--rotate", type=int, default=9,
                    help="distinct synthetic batches that take turns in the timed loop")
    ap.add_argument("--cu-split", choices=["cu", "xcd", "none"], default=None,
                    help="(DESIGN.md 5.4 probe, --backend gloo with ranks sharing a GPU) give every rank its own CUs through "
                         "HSA_CU_MASK before HIP starts: `cu` = a contiguous half of the mask bits, `xcd` = "
                         "the mask bits i with i %% 8 in its half of 0..7 (interleaved)")
    ap.add_argument("--no-profile", action="store_true",
                    help="do not bracket kernels with HIP events (roofline becomes null)")
    args = ap.parse_args()
    if args.dump_outputs and (args.dataset_images or args.host_images):
        ap.error("--dump-outputs writes the outputs of the timed steps: not with --dataset-images / --host-images")
    cu_mask = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        r, w = int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("LOCAL_WORLD_SIZE", os.environ["WORLD_SIZE"]))
        if args.cu_split in ("cu", "xcd"):   # (`none`: no mask at all -- the ranks share every CU; the probes of DESIGN.md 5.4: halves of the mask bits, or the bits i with i % 8 in a half)
            cus = range(r * 256 // w, (r + 1) * 256 // w) if args.cu_split == "cu" else \
                [i for i in range(256) if (i % 8) * w // 8 == r]
            cu_mask = os.environ["HSA_CU_MASK"] = "0:" + ",".join(str(i) for i in cus)
        elif args.cu_split is None:
            # ranks that share a GPU (the gloo dry run on a smaller box) get disjoint contiguous parts of the CU mask: before HIP starts
            # (the FILE, not the package: importing torch.distributed / RCCL already starts the runtime, and a mask set
            # after that is ignored)
            import importlib.util
            spec = importlib.util.spec_from_file_location("gpu_partition", os.path.join(ROOT, "lossyless_amd", "gpu_partition.py"))
            gp = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(gp)
            cu_mask = gp.partition_shared_gpu(r, w, if_unknown=1 if args.backend == "gloo" else 0)

    import numpy as np
    import torch
    import torch.distributed as dist
    import lossyless_amd  # noqa: F401  (its host-runtime settings must precede the first HIP call below)
    if int(os.environ.get("WORLD_SIZE", "1")) == 1:
        # a missing or STALE library (built from other sources than this tree's) is rebuilt here rather than measured;
        # under a launcher the ranks do not race to build: lib() raises there instead
        from lossyless_amd import _lib as _host_lib
        if _host_lib.ensure_built():
            print("bench.py: rebuilt " + _host_lib.LIB_PATH + " (it was missing or stale)", file=sys.stderr)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(respawn_under_torchrun(args.gpus))        # one process per GPU, this one only waits
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    ndev = torch.cuda.device_count()
    if world > ndev and args.backend == "nccl":
        raise SystemExit(f"--gpus {world} but only {ndev} GPU(s) visible: RCCL needs one GPU per rank "
                         "(--backend gloo dry-runs the N>1 code path on fewer GPUs)")
    dev_index = local_rank % max(ndev, 1)  # (% only matters for gloo dry runs on fewer GPUs)
    torch.cuda.set_device(dev_index)
    device = f"cuda:{dev_index}"
    comm = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # one rank's host side (enqueue thread, pinned staging, torch intra-op pool) on its own slice of the
        # node's cores: 8 ranks sharing one pool of 256 threads is the contention DESIGN.md section 6 measured
        # (98k -> 82k img/s per GPU with busy neighbours)
        from lossyless_amd import distributed as lla_dist_pin
        pinned = lla_dist_pin.pin_host_threads(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
        comm = dict(backend=args.backend, world_size=world, host_cpus_per_rank=pinned["cpus"],
                    torch_threads=pinned["threads"], host_numa_node=pinned["numa_node"], host_cpus_from=pinned["source"],
                    # (HSA_CU_MASK of this rank, abbreviated: the variable itself names every CU)
                    cu_mask=None if not cu_mask else "%s:%s..%s (%d CUs)" % (
                        cu_mask.split(":")[0], cu_mask.split(":")[1].split(",")[0], cu_mask.split(",")[-1],
                        len(cu_mask.split(","))))
        if args.backend == "nccl":   # RCCL over xGMI
            try:
                comm["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception as err:  # pragma: no cover
                comm["rccl_version"] = f"unavailable: {err!r}"
        if args.backend == "nccl":   # RCCL over xGMI
            dist.init_process_group("nccl", device_id=torch.device(device))
        else:                        # gloo: lets the N>1 code path be exercised on one GPU
            dist.init_process_group("gloo")

    base = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        base = cpu_baseline()

    import hubconf
    from lossyless_amd import distributed as lla_dist
    from lossyless_amd.clip_vit import KernelProfiler
    comp, _ = hubconf.clip_compressor_b005(device=device, clip_weights=os.environ.get(
        "LOSSYLESS_CLIP_WEIGHTS", "synthetic"), vit_chunk=args.chunk)
    if args.dataset_images:
        from lossyless_amd.compressor import SyntheticImages
        comp.device = device
        path = args.keep_file or os.path.join(os.environ.get("TMPDIR", "/tmp"), f"lla_bench_{os.getpid()}.bin")
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        comp.compress_dataset(SyntheticImages(args.dataset_images), path,
                              kwargs_dataloader=dict(batch_size=args.batch), is_info=False,
                              distributed=world > 1)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if rank == 0:
            import hashlib
            size = os.path.getsize(path)
            with open(path, "rb") as f:
                sha = hashlib.sha256(f.read()).hexdigest()
            if not args.keep_file:
                os.remove(path)
            print(json.dumps(dict(metric="compress_dataset_img_per_sec", file_sha256=sha, comm=comm,
                                  value=round(args.dataset_images / el, 1), unit="img/s",
                                  n_gpus=world, images=args.dataset_images, seconds=round(el, 3),
                                  bits_per_img=round(8 * size / args.dataset_images, 2),
                                  higher_is_better=True, data="synthetic (generated on device)",
                                  includes="generation + tower + entropy + gather + file write")))
        if world > 1:
            dist.destroy_process_group()
        return
    if args.host_images:
        # the same synthetic batch repeated, resident in pinned host memory; every batch crosses PCIe
        xb = synth_batch(args.batch, seed=rank, device=device).cpu()
        reps = (args.host_images + args.batch - 1) // args.batch
        host = torch.empty((reps * args.batch,) + tuple(xb.shape[1:]), dtype=xb.dtype).pin_memory()
        for r in range(reps):
            host[r * args.batch:(r + 1) * args.batch] = xb
        host = host[:args.host_images]
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"lla_bench_{os.getpid()}.bin")
        comp.device = device
        comp.compress_dataset(host[:2 * args.batch], path, kwargs_dataloader=dict(batch_size=args.batch),
                              is_info=False)                       # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        comp.compress_dataset(host, path, kwargs_dataloader=dict(batch_size=args.batch), is_info=False)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        size = os.path.getsize(path)
        os.remove(path)
        print(json.dumps(dict(metric="compress_dataset_host_fed_img_per_sec",
                              value=round(args.host_images / el, 1), unit="img/s", n_gpus=1,
                              images=args.host_images, seconds=round(el, 3),
                              bits_per_img=round(8 * size / args.host_images, 2),
                              host_bytes_per_img=int(host[0].numel() * host.element_size()),
                              pcie_gb_per_s=round(host.numel() * host.element_size() / el / 1e9, 2),
                              includes="pinned host fp16 NHWC -> H2D (one batch ahead on a side stream) "
                                       "+ tower + entropy + file write")))
        return
    entropy_model = "b005 frozen tables, shipped affine (all-escape case on synthetic tower weights)"
    shipped = (comp.scaling.detach().clone(), comp.biasing.detach().clone())    # hubconf.py:22-30 loads these
    calibrated = False
    if not args.shipped_affine and comp.clip_weights_desc == "synthetic-seed1":
        entropy_model = calibrate_affine_(comp, device)
        calibrated = True
    # --rotate distinct batches take turns in the timed loop (one tensor pushed every step can be served from the
    # 256-MB memory-side cache and always codes the same symbols); xs[0] is the batch the checker re-codes
    xs = synth_batches([(args.batch, rank + 131 * i) for i in range(max(args.rotate, 1))], device)
    if args.layout == "nchw":
        xs = [v.permute(0, 3, 1, 2).contiguous() for v in xs]
    x = xs[0]
    prof = KernelProfiler(max_launches=8192) if args.full and not args.no_profile else None

    def step(profiler=None):
        z = comp.clip(x, profiler=profiler)
        payload, offsets, _ = comp.entropy_bottleneck.encode_device(z, comp._tables(),
                                                                    record_prefix=True)
        total = int(offsets[-1])                    # the one device->host sync per batch
        return payload[:total].cpu().numpy()

    # The timed loop is the loop of compress_dataset: a RecordStream that runs the tower per batch
    # and entropy-codes the parked embeddings every `--entropy-group` batches and at the end
    # (finish() is inside the timed region, so every byte of every timed batch is produced there).
    # (under nccl the ranks that only send keep their records on the GPU: the gather reads them from HBM)
    stream = comp.record_stream(args.entropy_group, on_device=world > 1 and lla_dist.sends_from_device(device))
    for k in range(args.warmup):
        stream.push(xs[k % len(xs)], donate=True)
    stream.finish()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Timed region = `blocks` blocks of EXACTLY --steps steps each, back to back.  One block when --min-seconds is 0;
    # otherwise as many as it takes to (a) end on a whole tower pass (the RecordStream gathers steps into passes of
    # 8704 images: 20 steps = 2.4 passes, and a run that ends on a partial pass reads 2-4 % low) and (b) last
    # --min-seconds (a 0.2 s region is mostly pipeline fill and drain).  `value` = images actually timed / time.
    from lossyless_amd.compressor import _TOWER_BATCH as _PASS
    blocks = 1
    if args.min_seconds > 0 and args.entropy_group:
        import math
        fence()
        t0 = time.perf_counter()
        for k in range(4):
            stream.push(xs[k % len(xs)], donate=True)
        stream.finish()
        torch.cuda.synchronize()
        est = max((time.perf_counter() - t0) / 4, 1e-4)          # generous (includes a drain): only sizes the region
        per_block = args.steps * args.batch
        whole = _PASS // math.gcd(per_block, _PASS) if args.batch < _PASS else 1   # blocks per whole number of passes
        need = max(1, math.ceil(args.min_seconds / (est * args.steps)))
        blocks = -(-need // whole) * whole
        if world > 1:   # every rank must time the same number of images
            tb = torch.tensor([blocks], dtype=torch.int64, device=device if args.backend == "nccl" else "cpu")
            dist.all_reduce(tb, op=dist.ReduceOp.MAX)
            blocks = int(tb.item())
    fence()
    t0 = time.perf_counter()
    for k in range(blocks * args.steps):
        stream.push(xs[k % len(xs)], donate=True)
    body = stream.finish()
    n_local = args.batch * args.steps * blocks
    if world > 1:  # once per dataset: RCCL gather of the bitstream to rank 0
        body, _, n_all = lla_dist.gather_to_rank0(body, np.zeros(0, np.uint16), n_local, device)
    else:
        n_all = n_local
    local_elapsed = time.perf_counter() - t0     # this rank's own clock (before the closing barrier): stragglers show
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, body, n_all, world, args.batch)

    # Per-kernel HIP-event timing: the same steps again with every launch bracketed by events
    # on the launch stream.  Kept out of the region `value` is computed from because the event
    # records break back-to-back dispatch (~10 % slower end to end).
    # The launches timed here are the launches of the timed region: the RecordStream gathers the pushed batches
    # into tower passes of `tower_batch` images (8704 by default), so the profiled passes run on that many images
    # (the same batch, repeated).
    from lossyless_amd.compressor import _TOWER_BATCH
    tower_batch = max(_TOWER_BATCH, args.batch) if args.entropy_group else args.batch
    n_prof = max(1, min(args.steps * args.batch // tower_batch, 12))   # (the event pool holds 8192 launches; a pass has ~90)
    if prof:
        reps = -(-tower_batch // args.batch)
        xp = torch.cat([xs[k % len(xs)] for k in range(reps)])[:tower_batch] if reps > 1 else x
        comp.clip(xp, profiler=prof)
        prof.collect()
        for _ in range(n_prof):
            comp.clip(xp, profiler=prof)
        torch.cuda.synchronize()

    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # who ran where, and how fast on its own clock: the first N > 1 run must show N DISTINCT GPUs and any straggler
        mine = dict(rank=rank, local_rank=local_rank, img_per_sec=round(n_local / local_elapsed, 1),
                    seconds=round(local_elapsed, 4), host_cpus=comm["host_cpus_per_rank"], host_numa_node=comm["host_numa_node"],
                    host_cpus_from=comm["host_cpus_from"], cu_mask=comm["cu_mask"], **device_identity(dev_index))
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
        comm["ranks"] = per_rank
        ids = [r["pci_bus_id"] or r["uuid"] or r["device"] for r in per_rank]
        comm["distinct_devices"] = len(set(ids))

    roof = None
    if prof:
        c = prof.collect()["gemm"]
        if c["launches"]:
            achieved = c["work"] / (c["ms"] * 1e-3) / 1e12
            roof = dict(bound="mfma", kernel="gemm_w8_kernel / gemm_q4_kernel (GEMM class: every tower GEMM launch, all epilogues)",
                        achieved=round(achieved, 1), peak=PEAK_FP16_TFLOPS, unit="TFLOP/s",
                        frac=round(achieved / PEAK_FP16_TFLOPS, 4),
                        launches=c["launches"],
                        avg_launch_us=round(1e3 * c["ms"] / c["launches"], 2),
                        flop_per_launch=round(c["work"] / c["launches"]),
                        gemm_ms_per_step=round(c["ms"] / n_prof * args.batch / tower_batch, 3),
                        images_per_launch=tower_batch,
                        traffic=_pmc_traffic(tower_batch),
                        algorithmic_bytes_per_launch=round(gemm_algorithmic_bytes_per_launch(tower_batch)),
                        # what the large GEMMs are actually bound by: the bytes a CU's
                        # vector-memory path moves -- LDS-DMA operand stream + epilogue loads / stores of the 256 x 256
                        # tiles -- per second of GEMM time; every large GEMM of the tower sits at ~37 GB/s per CU
                        cu_vector_memory=dict(
                            bytes_per_row_tile_and_layer=VMEM_BYTES_PER_ROW_TILE_LAYER,
                            achieved_GBps_per_cu=round(VMEM_BYTES_PER_ROW_TILE_LAYER * 12 / 5.12 * tower_batch * c["launches"] / 51
                                                       / (c["ms"] * 1e-3) / 256 / 1e9, 2),
                            note="operand stream (64 KB per K-tile) + epilogue bytes of QKV / c_fc / out-proj / c_proj per 256-row "
                                 "tile and layer, x 12 layers / 5.12 images per row tile, / GEMM-class time / 256 CUs"),
                        timing="HIP events per launch on the launch stream, extra passes of the timed size after the timed region")
        prof.close()

    # The literal shipped clip_compressor_b005 (hubconf.py:22-30: the checkpoint's own scaling / biasing) on the same
    # batches: one more timed block of whole tower passes lasting >= 1 s.  With synthetic tower weights nearly every
    # symbol escapes the coding window (the coder's worst case); the tower's work is the same.
    shipped_line = None
    if args.full and calibrated and world == 1 and args.entropy_group:
        import math
        fitted = (comp.scaling.detach().clone(), comp.biasing.detach().clone())
        with torch.no_grad():
            comp.scaling.copy_(shipped[0]); comp.biasing.copy_(shipped[1])
        per_pass = max(_PASS // math.gcd(args.batch, _PASS), 1)          # steps per whole number of passes
        n_steps = -(-max(int(1.0 / (elapsed / (args.steps * blocks))), 1) // per_pass) * per_pass
        st2 = comp.record_stream(args.entropy_group)
        for k in range(per_pass):
            st2.push(xs[k % len(xs)], donate=True)
        st2.finish()
        fence()
        t1 = time.perf_counter()
        for k in range(n_steps):
            st2.push(xs[k % len(xs)], donate=True)
        body2 = st2.finish()
        fence()
        el2 = time.perf_counter() - t1
        shipped_line = dict(img_per_sec=round(n_steps * args.batch / el2, 1), seconds=round(el2, 4), steps=n_steps,
                            bits_per_img=round(8 * (4 + body2.size) / (n_steps * args.batch), 2))
        del st2, body2
        with torch.no_grad():
            comp.scaling.copy_(fitted[0]); comp.biasing.copy_(fitted[1])

    verified = None
    if args.full and rank == 0 and not args.no_verify:
        verified = verify_first_batch(comp, x)

    ent = pre = hyp = stl = rn = refcall = None
    if args.full and rank == 0 and world == 1 and not args.no_extra:
        ent = entropy_stage_leg(comp, device)
        pre = preprocess_leg(comp, device)
        hyp = hyperprior_leg(device)
        stl = stl10_shaped_leg(comp, device)
        refcall = reference_call_leg(device)
        rn = rn50_leg(device)

    if rank == 0:
        filesize = 4 + body.size
        ok = None if verified is None else bool(verified["records_equal_oracle"] and verified.get("embedding_ok", True))
        bits = round(8 * filesize / n_all, 2)
        # One line; what every field means is in DESIGN.md section 6 ("the bench line").  The driver's parser keeps the
        # contract keys and the config / roofline / cpu_baseline objects, so the figures a reader checks first ride in
        # `config` as flat numbers, and no string is longer than 100 characters.
        out = dict(
            metric="encode_img_per_sec", value=round(n_all / elapsed, 1), unit="img/s",
            n_gpus=world, steps=args.steps, warmup=args.warmup,
            ms_per_step=round(1e3 * elapsed / (args.steps * blocks), 3), higher_is_better=True,
            scaling="weak", vs_baseline=None, dtype="f16", data="synthetic",
            config=dict(workload=f"clip_compressor_b005 encode, synthetic 224x224x3 fp16 {args.layout.upper()}, "
                                 f"batch={args.batch}/GPU (configs[1])",
                        batch_per_gpu=args.batch, layout=args.layout, vit_weights=comp.clip_weights_desc,
                        entropy_model=entropy_model, parallelism=f"image-parallel x{world}",
                        entropy_group=args.entropy_group, tower_batch=tower_batch, tower_streams=1,
                        distinct_batches=len(xs), verified=ok, bits_per_img=bits,
                        timed_seconds=round(elapsed, 4), timed_steps=args.steps * blocks, timed_images=n_all,
                        shipped_affine_img_per_sec=None if shipped_line is None else shipped_line["img_per_sec"],
                        shipped_affine_bits_per_img=None if shipped_line is None else shipped_line["bits_per_img"]),
            roofline=roof, cpu_baseline=base,
            verified=ok, bits_per_img=bits, shipped_affine=shipped_line,
            timed_region=dict(blocks=blocks, steps_per_block=args.steps, steps=args.steps * blocks,
                              images_per_gpu=n_local, images=n_all, seconds=round(elapsed, 4),
                              tower_passes_per_gpu=round(n_local / max(_PASS, args.batch), 3)),
            tower_tflops=round(FLOP_PER_IMG * n_all / elapsed / 1e12, 1),
            verification=verified, comm=comm, entropy_stage=ent, preprocess_stage=pre,
            hyperprior_coder_stage=hyp, stl10_shaped_stage=stl, reference_call_stage=refcall, rn50_stage=rn,
            configs_2_3_4="tests/test_gpu_configs.py on generated stand-ins; reference's recorded numbers asset-gated")
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def entropy_stage_leg(comp, device, B=1024, iters=20):
    """Entropy stage alone on symbols drawn from the model's own pmf: with
    random ViT weights most embeddings escape the coding window, so the headline bits/img is
    not representative; here the payload should sit near sum_c H(pmf_c) + flush + length."""
    import numpy as np
    import torch
    from lossyless_amd import _lib
    t = comp._tables()
    cdf = t["cdf"].cpu().numpy()
    cdf_len = t["cdf_len"].cpu().numpy()
    off = t["offset"].cpu().numpy()
    rng = np.random.default_rng(2)
    C = cdf.shape[0]
    sym = np.empty((B, C), np.int32)
    for c in range(C):
        n = int(cdf_len[c])
        f = np.diff(cdf[c, :n]).astype(np.float64) / 65536.0
        v = rng.choice(n - 1, size=B, p=f)
        esc = v == n - 2                      # escape symbol: code an out-of-window neighbour
        v = np.where(esc, np.where(rng.integers(0, 2, B) == 0, -1, n - 2), v)
        sym[:, c] = v + off[c]
    L = _lib.lib()
    s = torch.from_numpy(sym).to(device)
    stride = int(L.lla_rans_max_encoded_bytes(C))
    scratch = torch.empty(B * stride, dtype=torch.uint8, device=device)
    lengths = torch.empty(B, dtype=torch.int32, device=device)
    eb = comp.entropy_bottleneck

    def once():
        rc = L.lla_rans_encode_batch(_lib.ptr(s), B, C, _lib.ptr(t["cdf"]), t["W"], _lib.ptr(t["cdf_len"]),
                                     _lib.ptr(t["offset"]), _lib.ptr(scratch), stride, _lib.ptr(lengths),
                                     _lib.stream_ptr(device))
        _lib.check(rc, "lla_rans_encode_batch")
        return eb.compact_device(scratch, stride, lengths, B, record_prefix=True)

    payload, offsets = once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        payload, offsets = once()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    total = int(offsets[-1])
    # decode side (lla_rans_decode_batch + lla_dequantise) on the same records
    back, status = eb.decode_device(payload, offsets, B, t, record_prefix=True)
    assert int(status.max()) == 0 and torch.equal(back, s)
    zh = torch.empty((B, C), dtype=torch.float32, device=device)
    e0.record()
    for _ in range(iters):
        back, status = eb.decode_device(payload, offsets, B, t, record_prefix=True)
        L.lla_dequantise(_lib.ptr(back), B, C, _lib.ptr(t["bias"]), _lib.ptr(t["exp_scale"]),
                         _lib.ptr(t["median"]), _lib.ptr(zh), _lib.stream_ptr(device))
    e1.record()
    torch.cuda.synchronize()
    dec_ms = e0.elapsed_time(e1) / iters
    # the same at the batch decompress_dataset decodes with (65536 records per call): the coder walks a
    # 512-symbol dependency chain per image with one image per lane, so batch 1024 keeps 16 of the chip's
    # 1024 SIMDs busy for the same ~0.3 ms that 65536 images take
    Bd = 65536
    sd = s.repeat(Bd // B, 1).contiguous()
    scr = torch.empty(Bd * stride, dtype=torch.uint8, device=device)
    lens = torch.empty(Bd, dtype=torch.int32, device=device)
    _lib.check(L.lla_rans_encode_batch(_lib.ptr(sd), Bd, C, _lib.ptr(t["cdf"]), t["W"], _lib.ptr(t["cdf_len"]),
                                       _lib.ptr(t["offset"]), _lib.ptr(scr), stride, _lib.ptr(lens),
                                       _lib.stream_ptr(device)), "lla_rans_encode_batch")
    payd, offd = eb.compact_device(scr, stride, lens, Bd, record_prefix=True)
    zhd = torch.empty((Bd, C), dtype=torch.float32, device=device)
    backd, std = eb.decode_device(payd, offd, Bd, t, record_prefix=True)
    assert int(std.max()) == 0 and torch.equal(backd, sd)
    e0.record()
    for _ in range(5):
        backd, std = eb.decode_device(payd, offd, Bd, t, record_prefix=True)
        L.lla_dequantise(_lib.ptr(backd), Bd, C, _lib.ptr(t["bias"]), _lib.ptr(t["exp_scale"]),
                         _lib.ptr(t["median"]), _lib.ptr(zhd), _lib.stream_ptr(device))
    e1.record()
    torch.cuda.synchronize()
    dec_ms_big = e0.elapsed_time(e1) / 5
    # the HOST coder on the same 65536 records: what decompress_dataset(is_cpu=True), the reference's default,
    # decodes with (lla_rans_decode_batch_host + lla_dequantise_host, threaded over images; no GPU involved)
    import ctypes
    body = payd[:int(offd[-1])].cpu().numpy()
    off_h = offd.cpu().numpy().astype(np.uint64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cdf_h = np.ascontiguousarray(cdf, dtype=np.int32)
    len_h, offs_h = np.ascontiguousarray(cdf_len, dtype=np.int32), np.ascontiguousarray(off, dtype=np.int32)
    sym_h = np.empty((Bd, C), np.int32)
    st_h = np.zeros(Bd, np.int32)
    z_h = np.empty((Bd, C), np.float32)
    bias_h, es_h, med_h = (t[k].cpu().numpy() for k in ("bias", "exp_scale", "median"))
    t_h = time.perf_counter()
    _lib.check(L.lla_rans_decode_batch_host(P(body), P(off_h), 1, Bd, C, P(cdf_h), t["W"], P(len_h), P(offs_h),
                                            P(sym_h), P(st_h)), "lla_rans_decode_batch_host")
    _lib.check(L.lla_dequantise_host(P(sym_h), Bd, C, P(bias_h), P(es_h), P(med_h), P(z_h)), "lla_dequantise_host")
    host_s = time.perf_counter() - t_h
    assert int(st_h.max()) == 0 and np.array_equal(sym_h[:B], sym)
    del sd, scr, lens, payd, offd, zhd, backd
    algo_bytes = B * C * 4 + total                # int32 symbols in + records out
    gbs = algo_bytes / (ms * 1e-3) / 1e9
    return dict(symbols="model pmf, seed 2", images=B, bits_per_img=round(8 * (total + 4) / B, 2),
                img_per_sec=round(B / (ms * 1e-3), 1), ms_per_batch=round(ms, 4),
                decode_img_per_sec=round(B / (dec_ms * 1e-3), 1),
                decode_img_per_sec_batch_65536=round(Bd / (dec_ms_big * 1e-3), 1),
                host_decode_img_per_sec=round(Bd / host_s, 1),
                roofline=dict(bound="hbm", achieved=round(gbs, 2), peak=8000.0, unit="GB/s",
                              frac=round(gbs / 8000.0, 6),
                              note="true bound is the 512-step rANS dependency chain x images in flight"))


def hyperprior_leg(device, B=1024, C=512, iters=10):
    """SURVEY.md 8(f) rank 4 coder: GaussianConditional strings (arbitrary table row per symbol,
    lla_rans_encode_indexed / _decode_indexed) for B rows of C symbols drawn from N(0, scale) with
    scales spread over the 64-level table; checked against the round trip."""
    import math
    import torch
    from lossyless_amd import _lib
    from lossyless_amd.entropy import EntropyBottleneck, GaussianConditional
    from lossyless_amd.rates import get_scale_table
    g = GaussianConditional(None).to(device).eval()
    g.update_scale_table(get_scale_table())
    t = g.device_tables()
    gen = torch.Generator().manual_seed(4)
    scales = torch.exp(torch.rand(B, C, generator=gen) * (math.log(256) - math.log(0.11)) + math.log(0.11))
    sym = torch.round(torch.randn(B, C, generator=gen) * scales).to(torch.int32).to(device)
    idx = g.build_indexes(scales.to(device)).contiguous()
    L = _lib.lib()
    stride = int(L.lla_rans_max_encoded_bytes(C))
    scratch = torch.empty(B * stride, dtype=torch.uint8, device=device)
    lengths = torch.empty(B, dtype=torch.int32, device=device)
    out = torch.empty((B, C), dtype=torch.int32, device=device)
    status = torch.zeros(B, dtype=torch.int32, device=device)

    def enc():
        rc = L.lla_rans_encode_indexed(_lib.ptr(sym), _lib.ptr(idx), B, C, _lib.ptr(t["cdf"]), t["T"], t["W"],
                                       _lib.ptr(t["cdf_len"]), _lib.ptr(t["offset"]), _lib.ptr(scratch),
                                       stride, _lib.ptr(lengths), _lib.stream_ptr(device))
        _lib.check(rc, "lla_rans_encode_indexed")
        return EntropyBottleneck.compact_device(scratch, stride, lengths, B)

    def dec(payload, offsets):
        rc = L.lla_rans_decode_indexed(_lib.ptr(payload), _lib.ptr(offsets), 0, B, C, _lib.ptr(idx),
                                       _lib.ptr(t["cdf"]), t["T"], t["W"], _lib.ptr(t["cdf_len"]),
                                       _lib.ptr(t["offset"]), _lib.ptr(out), _lib.ptr(status),
                                       _lib.stream_ptr(device))
        _lib.check(rc, "lla_rans_decode_indexed")

    payload, offsets = enc()
    dec(payload, offsets)
    torch.cuda.synchronize()
    assert int(status.max()) == 0 and torch.equal(out, sym)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        payload, offsets = enc()
    e1.record()
    torch.cuda.synchronize()
    ms_enc = e0.elapsed_time(e1) / iters
    e0.record()
    for _ in range(iters):
        dec(payload, offsets)
    e1.record()
    torch.cuda.synchronize()
    ms_dec = e0.elapsed_time(e1) / iters
    return dict(coder="GaussianConditional, 64-level scale table (T x W = %d x %d int32 in HBM)" % (t["T"], t["W"]),
                rows=B, symbols_per_row=C, bits_per_row=round(8 * int(offsets[-1]) / B, 2),
                encode_rows_per_sec=round(B / (ms_enc * 1e-3), 1), encode_ms=round(ms_enc, 4),
                decode_rows_per_sec=round(B / (ms_dec * 1e-3), 1), decode_ms=round(ms_dec, 4))


def preprocess_leg(comp, device, B=1024, H=96, W=96, iters=20):
    """GPU twin of the reference's PIL transform on STL10-shaped uint8 images (BASELINE
    configs[0] input shape): resize 96->224 bicubic + normalise -> fp16 NHWC.  HBM bound."""
    import torch
    g = torch.Generator().manual_seed(3)
    raw = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(device)
    out = comp.preprocess_gpu(raw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        comp.preprocess_gpu(raw, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    algo = B * (H * W * 3 + 224 * 224 * 3 * 2)          # u8 in + fp16 out (intermediate excluded)
    gbs = algo / (ms * 1e-3) / 1e9
    return dict(input=f"{B} x {H}x{W}x3 uint8", img_per_sec=round(B / (ms * 1e-3), 1),
                roofline=dict(bound="hbm", achieved=round(gbs, 1), peak=8000.0, unit="GB/s",
                              frac=round(gbs / 8000.0, 4)))


def stl10_shaped_leg(comp, device, n=32768, batch=1024, workers=0):
    """BASELINE configs[0] input shape on the GPU path: `compress_dataset` over STL10-shaped raw uint8
    96x96x3 images held on the HOST -- (a) a map-style dataset behind a DataLoader, as the reference is
    driven (hub/compressor.py:155,186), (b) the tensor fast path (pinned uint8 batches, one ahead) --
    resize 96->224 + normalise on the GPU (Pillow-exact), tower, entropy stage, file written."""
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (n, 96, 96, 3), generator=g, dtype=torch.uint8)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return n

        def __getitem__(self, i):
            return raw[i], i % 10

    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"lla_bench_stl_{os.getpid()}.bin")
    out = {}
    # (a): with num_workers=0 the 1024 __getitem__ calls + default_collate of a batch are host time in the main
    # process (compress_dataset caps torch's intra-op threads there: with the default 128-256 threads this leg
    # ran at 26k img/s, with 4 at 86-91k).  (b) is the path for data that is already a tensor.  The pinned copy of
    # (b) is made after (a) and dropped at the end: pinned pages are copied eagerly by every fork(), so a
    # process that keeps a pinned GiB around pays ~0.7 s per DataLoader worker it starts afterwards.
    for name, kw in (("dataloader", dict(batch_size=batch, num_workers=workers)),
                     ("tensor_fast_path", dict(batch_size=batch))):
        ds = DS() if name == "dataloader" else raw.pin_memory()
        comp.compress_dataset(raw[:batch] if name != "dataloader" else torch.utils.data.Subset(ds, range(batch)),
                              path, kwargs_dataloader=kw, is_info=False)          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        comp.compress_dataset(ds, path, kwargs_dataloader=kw, is_info=False)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        del ds
        out[name + "_img_per_sec"] = round(n / el, 1)
    out["bits_per_img"] = round(8 * os.path.getsize(path) / n, 2)
    os.remove(path)
    if hasattr(torch._C, "_host_emptyCache"):
        torch._C._host_emptyCache()
    out["input"] = f"{n} x 96x96x3 uint8 on the host (configs[0] shape), batch {batch}, num_workers={workers}"
    return out


def reference_call_leg(device, n=32768):
    """The reference's own call, unchanged (README / hub/compressor.py:150-207): a torchvision-style dataset built
    with the returned ``transform`` -- STL10-shaped: uint8 [N,3,96,96] in memory, ``__getitem__`` makes a PIL image
    and applies the transform (tools/workloads.py) -- handed to ``compress_dataset(dataset, file, label_file,
    kwargs_dataloader)`` with the reference's default loader arguments (batch 128, 16 workers) and with batches of
    1024.  (a) the PIL transform (resize / crop / normalise per image on the host: what the reference does),
    (b) ``gpu_preprocess=True`` (the transform hands the raw pixels over, the same chain runs on the GPU,
    bit-identical records).  Every setting is run at two sizes: the whole-call rate of the larger run (worker
    start-up included: 0.7-0.9 s for 16 workers.  This leg read 15 s per call until the GPU stalls that fork()
    causes through userptr-registered host memory were removed: DESIGN.md section 6, lossyless_amd/__init__.py) and the MARGINAL rate (images added / seconds added)."""
    import hashlib
    import torch
    import hubconf
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from workloads import Stl10Shaped
    out = dict(input="STL10-shaped images (uint8 [N,3,96,96] in host memory), labels written")
    tmp = os.environ.get("TMPDIR", "/tmp")
    path, lpath = os.path.join(tmp, f"lla_ref_{os.getpid()}.bin"), os.path.join(tmp, f"lla_ref_{os.getpid()}.npy")
    sha = {}
    full = Stl10Shaped(n, None)
    for gpu_pre, tag in ((False, "pil_transform"), (True, "gpu_preprocess")):
        comp, transform = hubconf.clip_compressor_b005(device=device, clip_weights=os.environ.get(
            "LOSSYLESS_CLIP_WEIGHTS", "synthetic"), gpu_preprocess=gpu_pre)
        full.transform = transform
        for kw in (dict(batch_size=128, num_workers=16), dict(batch_size=1024, num_workers=16)):
            if not gpu_pre and kw["batch_size"] != 128:
                continue
            sizes = (n // 8, n) if gpu_pre else (n // 32, n // 8)     # (the PIL path is ~10x slower: fewer images)
            secs = []
            for m in sizes:
                sub = full if m == n else torch.utils.data.Subset(full, range(m))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                comp.compress_dataset(sub, path, label_file=lpath, kwargs_dataloader=kw, is_info=False)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
            key = f"{tag}_batch{kw['batch_size']}_workers16"
            out[key] = dict(images=sizes[1], whole_call_img_per_sec=round(sizes[1] / secs[1], 1),
                            marginal_img_per_sec=round((sizes[1] - sizes[0]) / max(secs[1] - secs[0], 1e-9), 1),
                            seconds=[round(v, 2) for v in secs])
            if sizes[1] == n:
                with open(path, "rb") as f:
                    sha[key] = hashlib.sha256(f.read()).hexdigest()
        if gpu_pre:   # the literal README call: no loader arguments at all
            for m, key in ((8000, "gpu_preprocess_default_arguments"), (n, f"gpu_preprocess_default_arguments_{n}_images")):
                sub = full if m == n else torch.utils.data.Subset(full, range(m))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                comp.compress_dataset(sub, path, label_file=lpath, is_info=False)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                # (an in-memory array dataset whose transform is RawRGB is read straight from its array:
                # ClipCompressor._array_backed)
                out[key] = dict(images=m, whole_call_img_per_sec=round(m / el, 1), seconds=round(el, 3))
                if m == n:
                    with open(path, "rb") as f:
                        sha[key] = hashlib.sha256(f.read()).hexdigest()
            # the same call on a dataset the size of STL10's unlabeled split (100 000 images; here 3 x the 32 768): above
            # 12 288 images the default loader arguments are the reference's (batch 128, 16 workers)
            big = torch.utils.data.ConcatDataset([full, full, full])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            comp.compress_dataset(big, path, label_file=lpath, is_info=False)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            out["gpu_preprocess_default_arguments_98304_images"] = dict(
                images=len(big), whole_call_img_per_sec=round(len(big) / el, 1), seconds=round(el, 2))
            comp.compress_dataset(full, path, label_file=lpath, kwargs_dataloader=dict(batch_size=1024, num_workers=16),
                                  is_info=False)     # (leave the n-image file behind for bits_per_img below)
        del comp
    out["bits_per_img"] = round(8 * os.path.getsize(path) / n, 2)
    out["files_identical_across_loader_settings"] = len(set(sha.values())) == 1
    os.remove(path)
    os.remove(lpath)
    return out


def rn50_leg(device, B=1024, iters=3):
    """the RN50-CLIP visual tower (lossyless/architectures.py:367-371) on
    synthetic weights: 1x1 convolutions as GEMMs over the NHWC activations in place, 3x3 convolutions as implicit
    GEMMs (the loader gathers the taps) from 128 channels on and as direct convolutions (csrc/conv_direct.hip: a tile per
    wave, halo in LDS once) for the stem and layer1, ReLU / add+ReLU / average-pool epilogues."""
    import torch
    from lossyless_amd.clip_rn50 import ModifiedResNet, synthetic_rn50_state_dict
    net = ModifiedResNet(synthetic_rn50_state_dict(1), chunk=B).to(device)   # (20 MB of workspace per image)
    x = synth_batch(B, 7, device)
    net(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        net(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    from lossyless_amd.clip_rn50 import rn50_macs_per_image
    macs, stages = rn50_macs_per_image()
    tflops = 2.0 * macs * B / (ms * 1e-3) / 1e12
    return dict(images=B, img_per_sec=round(B / (ms * 1e-3), 1), ms_per_batch=round(ms, 3),
                gflop_per_img=round(2.0 * macs / 1e9, 4), gmac_by_stage={k: round(v / 1e9, 4) for k, v in stages.items()},
                roofline=dict(bound="mfma", achieved=round(tflops, 1), peak=PEAK_FP16_TFLOPS, unit="TFLOP/s",
                              frac=round(tflops / PEAK_FP16_TFLOPS, 4),
                              note="whole tower, algorithmic FLOPs; per-launch table profiles/r06_rn50_layer_table.txt, kernel table profiles/r06_rn50_kernel_stats.csv"),
                weights="synthetic-seed1")


def gemm_algorithmic_bytes_per_launch(images):
    """Algorithmic HBM bytes of one tower pass's GEMM launches (51 per pass of ViT-B/32 with the last block pruned to the
    class token), divided by their number: every operand read once, every output written once, the fp32 residual stream
    read and written by the two residual GEMMs of a block.  The denominator of `roofline.traffic`'s over-fetch ratio."""
    M, B = images * 50, images

    def gemm(m, n, k, resid=False):
        return m * k * 2 + n * k * 2 + (2 * m * n * 4 if resid else m * n * 2)
    ln_out = M * 768 * 2      # (round 5: the residual GEMMs of blocks 0-10 also write the LayerNorm output that follows them)
    block = gemm(M, 2304, 768) + gemm(M, 768, 768, True) + gemm(M, 3072, 768) + gemm(M, 768, 3072, True) + 2 * ln_out
    last = gemm(M, 1536, 768) + gemm(B, 768, 768) + gemm(B, 768, 768, True) + gemm(B, 3072, 768) + gemm(B, 768, 3072, True)
    patch = B * 224 * 224 * 3 * 2 + 768 * 3072 * 2 + B * 49 * 768 * 4      # (images read in place, fp32 token rows written)
    proj = gemm(B, 512, 768)
    return (11 * block + last + patch + proj) / (11 * 4 + 5 + 1 + 1)


def _pmc_traffic(images_per_launch=None):
    """HBM bytes per GEMM launch from the committed rocprofv3 --pmc passes (tools/profile_round.sh writes
    profiles/pmc_traffic.json with the sha of the kernel sources it profiled).  A profile taken on other kernel
    sources than the ones in this tree is STALE and not printed: null."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(p):
        try:
            with open(p) as f:
                d = json.load(f)
            if d.get("kernel_source_sha") != kernel_source_sha():
                return None
            if images_per_launch is not None and d.get("images_per_launch") != images_per_launch:
                return None      # counters of another launch mix (tower pass size) than the one timed here
            return d.get("gemm_bytes_per_launch")
        except Exception:
            return None
    return None


if __name__ == "__main__":
    main()
