"""BASELINE.json configs[2] / configs[4] harness: rate sweep over the three shipped rate points and
round trip + downstream accuracy, on real data when it is available.

    python tools/rate_sweep.py --images X.npy [--labels Y.npy] [--test-images Xt.npy --test-labels Yt.npy]
    python tools/rate_sweep.py --stl10-shaped          # configs[4] shape: 5 000 train / 8 000 test, 96x96, 10 classes
    python tools/rate_sweep.py --imagenet-shaped 50000 # configs[2] shape: 50 000 photos of mixed sizes

`X.npy`: uint8 images [N, H, W, 3] (e.g. STL10 96x96 or ImageNet-val resized); they go through the GPU
preprocessing (Pillow-exact resize / centre crop / CLIP normalisation) and `compress_dataset`.  With real CLIP
weights (`$LOSSYLESS_CLIP_WEIGHTS`) the numbers are comparable with the reference's (README.md:75,
notebooks/Hub.ipynb: 1506.6 bits/img and 98.64 % LinearSVC(C=7e-3) accuracy on STL10 at beta = 5e-2).
The two `-shaped` modes run the REFERENCE CALL -- a torchvision-style `Dataset(transform=transform)` handed to
`compress_dataset(dataset, file, label_file, kwargs_dataloader)` (hub/compressor.py:150-207) with the
compressor built with `gpu_preprocess=True` -- on generated stand-ins of the real datasets' shapes
(tools/workloads.py: the real files cannot be fetched offline), and say so in `data`.
Without real weights the output says so too: these runs exercise the path at the datasets' scale and shapes,
not the reference's numbers.  Prints one JSON line per rate point; `--device-bottleneck-fit BETA` adds a rate point trained
in the run (lossyless_amd.BottleneckFit on the tower's features of the training images) and its line,
`--device-hyperprior-fit BETA` the same with lossyless_amd.HyperpriorFit.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubconf  # noqa: E402


def _compress(comp, data, f, label_file, loader):
    t0 = time.perf_counter()
    comp.compress_dataset(data, f, label_file=label_file, kwargs_dataloader=loader, is_info=False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _represent(comp, data, idx, batch):
    """compressor(X) for the samples `idx` of a tensor or a dataset of raw images."""
    out = []
    for i in range(0, len(idx), batch):
        j = idx[i:i + batch]
        if isinstance(data, torch.Tensor):
            x = data[j].cuda()
        else:
            x = [data[int(k)][0] for k in j]          # raw uint8 [H,W,3] tensors of any size
        out.append(comp(x).cpu())
    return torch.cat(out).numpy()


def _features(comp, data, batch):
    """The tower's features (fp16 [N, 512] on the device) of a tensor or a dataset of raw images: what the rate model codes."""
    out = []
    with torch.no_grad():
        for i in range(0, len(data), batch):
            if isinstance(data, torch.Tensor):
                x = data[i:i + batch].cuda()
            else:
                x = [data[k][0] for k in range(i, min(i + batch, len(data)))]
            out.append(comp._embed(x))
    return torch.cat(out)


def _fit_leg(args, comp, train, data, weights, shaped, loader, hyperprior=False):
    """Train a rate point on the run's features -- BottleneckFit, or HyperpriorFit with ``hyperprior`` -- code the run's images
    with it, print its line."""
    from lossyless_amd import BottleneckFit, HyperpriorFit
    n = len(train)
    feats = _features(comp, train, args.batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if hyperprior:
        name, beta, epochs, key = "HyperpriorFit", args.device_hyperprior_fit, args.hyperprior_fit_epochs, "hyperprior_fit"
        fit = HyperpriorFit(beta, epochs=epochs, batch_size=min(1024, n)).fit(feats)
    else:
        name, beta, epochs, key = "BottleneckFit", args.device_bottleneck_fit, args.bottleneck_fit_epochs, "bottleneck_fit"
        fit = BottleneckFit(beta, epochs=epochs, batch_size=min(1024, n)).fit(feats)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    if hyperprior:
        fitted, _ = hubconf.clip_hyperprior_compressor(fit.state_dict(), device="cuda", clip_weights=weights,
                                                       gpu_preprocess=shaped, coded_means=args.coded_means)
    else:
        fitted, _ = hubconf.clip_compressor(fit.state_dict(), device="cuda", clip_weights=weights, gpu_preprocess=shaped)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "Z.bin")
        enc = _compress(fitted, train, f, None, loader)
        bits = 8 * os.path.getsize(f) / n
        Z = fitted.decompress_dataset(f, is_info=False)
        idx = np.arange(n) if (not shaped or n <= args.check) else np.linspace(0, n - 1, args.check).astype(np.int64)
        assert np.array_equal(Z[idx], _represent(fitted, train, idx, args.batch))
    line = {"rate_point": f"{name}(beta={beta:g})", "data": data, "clip_weights": weights, "images": n,
            "bits_per_img": round(bits, 2), "encode_img_per_sec": round(n / enc, 1), "round_trip": "exact",
            "round_trip_samples": int(len(idx)), f"{key}_s": round(fit_s, 3), f"{key}_epochs": fit.epochs,
            f"{key}_rate_curve_bits": [round(r, 2) for r in fit.rate_curve_],
            f"{key}_distortion_curve": [round(r, 5) for r in fit.distortion_curve_]}
    if hyperprior:
        line[f"{key}_side_rate_curve_bits"] = [round(r, 2) for r in fit.side_rate_curve_]
        line["coded_means"] = args.coded_means
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images")
    ap.add_argument("--labels")
    ap.add_argument("--test-images")
    ap.add_argument("--test-labels")
    ap.add_argument("--stl10-shaped", action="store_true")
    ap.add_argument("--imagenet-shaped", type=int, default=0, metavar="N")
    ap.add_argument("--n-synthetic", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--workers", type=int, default=16, help="DataLoader workers of the -shaped modes")
    ap.add_argument("--check", type=int, default=4096,
                    help="-shaped modes: samples whose decoded rows are compared with compressor(X)")
    ap.add_argument("--device-probe", action="store_true",
                    help="also fit lossyless_amd.LinearProbe on the device from the container kept compressed "
                         "(adds linear_probe_accuracy and linear_probe_fit_s)")
    ap.add_argument("--device-probe-cv", type=int, default=0, metavar="N",
                    help="also run the reference's search (utils/Z_linear_eval.py: N draws of C ~ loguniform(1e-3, 1) and "
                         "class_weight, 5-fold up to 50 000 rows, one train / validation split above) with "
                         "lossyless_amd.LinearProbeCV on the device (adds linear_probe_cv_best, _validation_accuracy, "
                         "_accuracy and _fit_s)")
    ap.add_argument("--device-logistic-cv", type=int, default=0, metavar="N",
                    help="also run CLIP's linear-probe protocol (softmax regression, N values of C log-spaced in [1e-3, 10], the "
                         "same folds as --device-probe-cv) with lossyless_amd.LogisticProbeCV on the device (adds "
                         "logistic_probe_cv_best, _validation_accuracy, _accuracy and _fit_s)")
    ap.add_argument("--device-mlp", action="store_true",
                    help="also train lossyless_amd.MLPProbe (the reference's MLP predictor at its class defaults: 2 x 2048 "
                         "hidden units, AdamW, 10 epochs of shuffled minibatches of 128) on the device from the container kept "
                         "compressed (adds mlp_probe_accuracy and mlp_probe_fit_s)")
    ap.add_argument("--device-mlp-config", action="store_true",
                    help="also train lossyless_amd.BatchNormMLPProbe (the reference's predictor as config/main.yaml wires it: "
                         "mlp_probe.yaml's batchnorm and dropout 0.2, AdamW lr 3e-4 wd 1e-5, unifmultistep100) the same way (adds "
                         "mlp_config_probe_accuracy and mlp_config_probe_fit_s)")
    ap.add_argument("--device-knn", action="store_true",
                    help="also run the training-free protocol, lossyless_amd.KNNProbe (weighted k-NN: cosine, k = 20, T = 0.07), "
                         "on the device from the container kept compressed (adds knn_probe_accuracy, the leave-one-out "
                         "knn_probe_train_accuracy and knn_probe_s)")
    ap.add_argument("--device-ridge", type=int, default=0, metavar="N",
                    help="also run lossyless_amd.RidgeProbeCV (scikit-learn's RidgeClassifier objective, N values of alpha "
                         "log-spaced in [1e-3, 1e3], 5 stratified folds, two walks of the container in all) on the device "
                         "(adds ridge_probe_cv_best, _validation_accuracy, _accuracy and _fit_s)")
    ap.add_argument("--device-zero-shot", default=None, metavar="TOKENS.npy",
                    help="also classify the test split with no training rows: lossyless_amd.ZeroShotProbe over the class "
                         "prompts' token ids [K, n_templates, T] in TOKENS.npy (class k = label k), embedded by the text tower "
                         "of $LOSSYLESS_CLIP_WEIGHTS on the device (adds zero_shot_accuracy, zero_shot_top5_accuracy and "
                         "zero_shot_s; with the synthetic weights the figure is the path's, not CLIP's)")
    ap.add_argument("--device-bottleneck-fit", type=float, default=0.0, metavar="BETA",
                    help="also train a rate point of its own with lossyless_amd.BottleneckFit(BETA) on the device, on the tower's "
                         "features of the run's training images, load its state_dict() through hubconf.clip_compressor and "
                         "code the same images with it (one more JSON line: bits_per_img, the fit's time and curves)")
    ap.add_argument("--bottleneck-fit-epochs", type=int, default=10)
    ap.add_argument("--device-hyperprior-fit", type=float, default=0.0, metavar="BETA",
                    help="the same with lossyless_amd.HyperpriorFit(BETA): the scale-hyperprior rate model trained on the device, "
                         "loaded through hubconf.clip_hyperprior_compressor (one more JSON line, with the side information's "
                         "share of the rate)")
    ap.add_argument("--hyperprior-fit-epochs", type=int, default=10)
    ap.add_argument("--coded-means", choices=("scales", "predicted"), default="scales",
                    help="--device-hyperprior-fit: code with the scales in the means' place (the reference's coder) or with the "
                         "predicted means the model was trained with (HRateHyperprior(coded_means=))")
    args = ap.parse_args()

    weights = os.environ.get("LOSSYLESS_CLIP_WEIGHTS", "synthetic")
    shaped = args.stl10_shaped or args.imagenet_shaped > 0
    loader = dict(batch_size=args.batch)
    Y = Yt = test = None
    if shaped:
        from workloads import MixedSizeImages, Stl10Shaped
        loader = dict(batch_size=args.batch, num_workers=args.workers)
    elif args.images:
        train = torch.from_numpy(np.load(args.images))
        data = os.path.basename(args.images)
        Y = np.load(args.labels) if args.labels else None
        test = torch.from_numpy(np.load(args.test_images)) if args.test_images else None
        Yt = np.load(args.test_labels) if args.test_labels else None
    else:
        g = torch.Generator().manual_seed(0)
        train = torch.randint(0, 256, (args.n_synthetic, 96, 96, 3), generator=g, dtype=torch.uint8)
        data = f"synthetic uint8 96x96 x{args.n_synthetic} (no --images: assets absent)"

    for name in ("clip_compressor_b01", "clip_compressor_b005", "clip_compressor_b001"):
        comp, transform = getattr(hubconf, name)(device="cuda", clip_weights=weights, gpu_preprocess=shaped)
        if args.stl10_shaped:
            train, test = Stl10Shaped(5000, transform, split_seed=0), Stl10Shaped(8000, transform, split_seed=1)
            Y, Yt = train.labels, test.labels
            data = "STL10-shaped stand-in: 5000 train / 8000 test generated 96x96 images, 10 classes (STL10 absent)"
        elif args.imagenet_shaped:
            train = MixedSizeImages(args.imagenet_shaped, transform)
            Y = train.targets
            data = (f"ImageNet-val-shaped stand-in: {args.imagenet_shaped} generated photos, "
                    f"{len(set(train.shape_of.tolist()))} sizes from 96x128 to 2448x3264 (ImageNet absent)")
        n = len(train)
        with tempfile.TemporaryDirectory() as d:
            f, lf = os.path.join(d, "Z.bin"), (os.path.join(d, "Y.npy") if shaped else None)
            enc = _compress(comp, train, f, lf, loader)
            bits = 8 * os.path.getsize(f) / n
            t0 = time.perf_counter()
            Z = comp.decompress_dataset(f, label_file=lf, is_info=False)
            dec = time.perf_counter() - t0
            if shaped:
                Z, Yfile = Z
                assert np.array_equal(Yfile, np.asarray(Y) % 65536)      # labels ride as uint16 (hub/compressor.py:189)
            assert Z.shape == (n, 512)
            # the file decodes to exactly what compressor(X) returns (all samples, or an evenly spread subset)
            idx = np.arange(n) if (not shaped or n <= args.check) else np.linspace(0, n - 1, args.check).astype(np.int64)
            ref = _represent(comp, train, idx, args.batch)
            assert np.array_equal(Z[idx], ref)
            acc = "skipped: labels / test split not given"
            probe = {}
            if Y is not None and test is not None and Yt is not None:
                from sklearn.svm import LinearSVC
                ft = os.path.join(d, "Zt.bin")
                _compress(comp, test, ft, None, loader)
                Zt = comp.decompress_dataset(ft, is_info=False)
                clf = LinearSVC(C=7e-3).fit(Z, Y)          # README.md:75
                acc = float(clf.score(Zt, Yt))
                if args.device_probe:
                    from lossyless_amd import LinearProbe
                    t0 = time.perf_counter()
                    fitted = LinearProbe(C=7e-3).fit(comp.open_dataset(f), np.asarray(Y))   # the same objective, on the device
                    torch.cuda.synchronize()
                    probe = dict(linear_probe_fit_s=round(time.perf_counter() - t0, 3),
                                 linear_probe_accuracy=float(fitted.score(comp.open_dataset(ft), np.asarray(Yt))))
                if args.device_probe_cv:
                    from lossyless_amd import LinearProbeCV
                    # above 50 000 rows the reference validates on one predefined split: every tenth row here
                    folds = 5 if n <= 50000 else np.where(np.arange(n) % 10 == 0, 0, -1)
                    t0 = time.perf_counter()
                    cv = LinearProbeCV(LinearProbeCV.sample(args.device_probe_cv, seed=0), cv=folds)
                    cv.fit(comp.open_dataset(f), np.asarray(Y))
                    torch.cuda.synchronize()
                    probe.update(linear_probe_cv_fit_s=round(time.perf_counter() - t0, 3),
                                 linear_probe_cv_best=dict(cv.best_params_),
                                 linear_probe_cv_validation_accuracy=float(cv.mean_scores_[cv.best_index_]),
                                 linear_probe_cv_accuracy=float(cv.best_estimator_.score(comp.open_dataset(ft), np.asarray(Yt))))
                if args.device_logistic_cv:
                    from lossyless_amd import LogisticProbeCV
                    folds = 5 if n <= 50000 else np.where(np.arange(n) % 10 == 0, 0, -1)
                    t0 = time.perf_counter()
                    cv = LogisticProbeCV(LogisticProbeCV.logspace(args.device_logistic_cv, 1e-3, 10.0), cv=folds)
                    cv.fit(comp.open_dataset(f), np.asarray(Y))
                    torch.cuda.synchronize()
                    probe.update(logistic_probe_cv_fit_s=round(time.perf_counter() - t0, 3),
                                 logistic_probe_cv_best=dict(cv.best_params_),
                                 logistic_probe_cv_validation_accuracy=float(cv.mean_scores_[cv.best_index_]),
                                 logistic_probe_cv_accuracy=float(cv.best_estimator_.score(comp.open_dataset(ft), np.asarray(Yt))))
                if args.device_mlp:
                    from lossyless_amd import MLPProbe
                    t0 = time.perf_counter()
                    mlp = MLPProbe().fit(comp.open_dataset(f), np.asarray(Y))
                    torch.cuda.synchronize()
                    probe.update(mlp_probe_fit_s=round(time.perf_counter() - t0, 3),
                                 mlp_probe_accuracy=float(mlp.score(comp.open_dataset(ft), np.asarray(Yt))))
                if args.device_mlp_config:
                    from lossyless_amd import BatchNormMLPProbe
                    t0 = time.perf_counter()
                    bn_mlp = BatchNormMLPProbe(scheduler="unifmultistep").fit(comp.open_dataset(f), np.asarray(Y))
                    torch.cuda.synchronize()
                    probe.update(mlp_config_probe_fit_s=round(time.perf_counter() - t0, 3),
                                 mlp_config_probe_accuracy=float(bn_mlp.score(comp.open_dataset(ft), np.asarray(Yt))))
                if args.device_knn:
                    from lossyless_amd import KNNProbe
                    t0 = time.perf_counter()
                    knn = KNNProbe(k=min(20, len(Y) - 1)).fit(comp.open_dataset(f), np.asarray(Y))
                    knn_accuracy = float(knn.score(comp.open_dataset(ft), np.asarray(Yt)))
                    knn_train = float(knn.score(None, exclude_self=True))
                    torch.cuda.synchronize()
                    probe.update(knn_probe_s=round(time.perf_counter() - t0, 3), knn_probe_accuracy=knn_accuracy,
                                 knn_probe_train_accuracy=knn_train)
                if args.device_ridge:
                    from lossyless_amd import RidgeProbeCV
                    t0 = time.perf_counter()
                    ridge = RidgeProbeCV(RidgeProbeCV.logspace(args.device_ridge, 1e-3, 1e3), cv=5).fit(comp.open_dataset(f), np.asarray(Y))
                    torch.cuda.synchronize()
                    probe.update(ridge_probe_cv_fit_s=round(time.perf_counter() - t0, 3), ridge_probe_cv_best=ridge.best_params_,
                                 ridge_probe_cv_validation_accuracy=float(ridge.mean_scores_.max()),
                                 ridge_probe_cv_accuracy=float(ridge.best_estimator_.score(comp.open_dataset(ft), np.asarray(Yt))))
                if args.device_zero_shot:
                    from lossyless_amd import ZeroShotProbe
                    t0 = time.perf_counter()
                    tokens = np.load(args.device_zero_shot)
                    zs = ZeroShotProbe.from_tokens(hubconf.clip_text_encoder(weights, device="cuda"), tokens)
                    zs_acc = float(zs.score(comp.open_dataset(ft), np.asarray(Yt)))
                    zs_top5 = float(zs.top_k_score(comp.open_dataset(ft), min(5, tokens.shape[0]), np.asarray(Yt)))
                    torch.cuda.synchronize()
                    probe.update(zero_shot_s=round(time.perf_counter() - t0, 3), zero_shot_accuracy=zs_acc,
                                 zero_shot_top5_accuracy=zs_top5)
        print(json.dumps(dict(rate_point=name, data=data, clip_weights=weights, images=n,
                              call=("Dataset(transform=RawRGB) -> compress_dataset(dataset, file, label_file, "
                                    f"dict(batch_size={args.batch}, num_workers={args.workers}))") if shaped
                              else "tensor fast path",
                              bits_per_img=round(bits, 2), encode_img_per_sec=round(n / enc, 1),
                              decode_img_per_sec=round(n / dec, 1), round_trip="exact",
                              round_trip_samples=int(len(idx)), linear_svc_accuracy=acc, **probe)), flush=True)
    if args.device_bottleneck_fit > 0:
        _fit_leg(args, comp, train, data, weights, shaped, loader)
    if args.device_hyperprior_fit > 0:
        _fit_leg(args, comp, train, data, weights, shaped, loader, hyperprior=True)


if __name__ == "__main__":
    main()
