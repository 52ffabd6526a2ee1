"""Generate the ordered-mode golden pair under tests/golden/ (run ON AN MI355X: the point is that the device wrote it).

  ordered_hyperprior.bin        pair container (be32(2N), then z / side records) of 32 seeded feature rows, written by
                                ``HRateHyperprior(512, mlp_precision="ordered").encode_device`` with the synthetic seed-0
                                state dict in its machine-independent form (tests/ordered_util.py ``golden_state_dict``)
  ordered_hyperprior_z_hat.npy  fp32 [32, 512]: what ``decode_device`` gave for it there

tests/test_ordered_mlp_host.py decodes the container on the host, tests/test_gpu_ordered_mlp.py on the device; both
compare bits with the array.  ``--out DIR`` writes somewhere else than tests/golden/.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ordered_util import golden_state_dict, mixed_rows  # noqa: E402
from lossyless_amd.rates import HRateHyperprior  # noqa: E402
from lossyless_amd.hyperprior_compressor import write_pair_container  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    m = HRateHyperprior(512, mlp_precision="ordered").eval()
    m.load_state_dict(golden_state_dict())
    m = m.cuda()
    z = mixed_rows(32, 512, seed=2).cuda()
    payload, offsets, sym = m.encode_device(z, want_symbols=True)
    z_hat = m.decode_device(payload, offsets, 32)
    assert torch.equal(z_hat, m.represent_device(z))
    off = offsets.cpu().numpy()
    blob = payload[:int(off[-1])].cpu().numpy().tobytes()
    rec = [blob[int(off[r]) + 4:int(off[r + 1])] for r in range(64)]
    write_pair_container(os.path.join(args.out, "ordered_hyperprior.bin"), rec[0::2], rec[1::2])
    np.save(os.path.join(args.out, "ordered_hyperprior_z_hat.npy"), z_hat.cpu().numpy())
    print("ordered golden:", int(off[-1]) + 4, "bytes,", sym["z_indexes"].unique().numel(), "table rows,",
          sym["side_symbols"].unique().numel(), "distinct side symbols")


if __name__ == "__main__":
    main()
