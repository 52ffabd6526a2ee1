"""torch.hub entry points with the reference's factory names and return shape
(reference hubconf.py:22-52): ``clip_compressor_b005``, ``clip_compressor_b001`` and
``clip_compressor_b01``, each ``(device=..., **kwargs) -> (compressor, transform)``; ``clip_compressor(state_dict)`` and
``clip_hyperprior_compressor(state_dict)`` take a rate point of the caller's; ``feature_compressor(state_dict)`` is the
same dataset surface for a matrix of features from any other encoder, at the width the state dict has.

The reference fetches one state-dict per rate point from its GitHub release
(hubconf.py:15,23-26).  Here the three state-dicts ship inside the package with their integer
coding tables already frozen (``lossyless_amd/assets``), so nothing is
fetched; the release URL is only a fallback for a missing asset.
``clip_compressor(state_dict)`` takes any other factorized rate point: one trained here with
``lossyless_amd.BottleneckFit`` on frozen features, or a ``main.py`` checkpoint's rate estimator.
"""
dependencies = ["torch", "numpy"]

import pathlib

import torch

from lossyless_amd import ClipCompressor as _Compressor
from lossyless_amd import HyperpriorClipCompressor as _HyperpriorCompressor
from lossyless_amd import FeatureCompressor as _FeatureCompressor

_ASSET_DIR = pathlib.Path(__file__).resolve().parent / "lossyless_amd" / "assets"
_ASSET_NAME = "beta{beta:0.0e}_factorized_rate.pt"
_RELEASE = "https://github.com/YannDubs/lossyless/releases/download/v1.0/" + _ASSET_NAME
_ON = "cuda" if torch.cuda.is_available() else "cpu"

_DOC = """CLIP ViT-B/32 + entropy bottleneck compressor at beta = {beta:.0e}, MI355X kernels.

    device       : "cuda" (coding runs on the GPU only; there is no CPU fallback)
    clip_weights : path to OpenAI ViT-B-32.pt / a visual state-dict; default $LOSSYLESS_CLIP_WEIGHTS.
                   REQUIRED one way or the other (ValueError otherwise: the rate models only make
                   sense on real CLIP features); "synthetic" = seed-1 random weights, tests/bench only
    gpu_preprocess : False (default) -> ``transform`` is the reference's PIL chain (resize to 224, centre crop,
                   CLIP normalisation, on the host per image); True -> ``transform`` only hands the raw RGB
                   pixels over and the same chain runs on the GPU (bit-identical) inside
                   ``compress_dataset`` / ``compressor(X)`` -- the unchanged reference call
                   ``STL10(transform=transform)`` + ``compress_dataset(dataset, ...)`` then runs at GPU speed
    other kwargs : forwarded to ``lossyless_amd.ClipCompressor``

    Returns ``(compressor, transform)``: ``compressor(X)`` -> reconstructed representations,
    ``compressor.compress(X)`` -> byte strings, ``compress_dataset`` / ``decompress_dataset`` for
    whole datasets (the reference's ``.bin`` format); ``transform`` = resize to 224, centre crop,
    CLIP normalisation.
    """


def _weights_for(beta):
    asset = _ASSET_DIR / _ASSET_NAME.format(beta=beta)
    if asset.exists():
        return torch.load(asset, map_location="cpu", weights_only=True)
    return torch.hub.load_state_dict_from_url(_RELEASE.format(beta=beta), progress=False)


def _entry(tag, beta):
    def factory(device=_ON, **kwargs):
        model = _Compressor(pretrained_state_dict=_weights_for(beta), device=device, **kwargs)
        return model, model.preprocess
    factory.__name__ = factory.__qualname__ = "clip_compressor_" + tag
    factory.__doc__ = _DOC.format(beta=beta)
    return factory


clip_compressor_b005 = _entry("b005", 5e-2)
clip_compressor_b001 = _entry("b001", 1e-2)
clip_compressor_b01 = _entry("b01", 1e-1)


def clip_hyperprior_compressor(state_dict, device=_ON, coded_means="scales", mlp_precision="fp32", **kwargs):
    """CLIP ViT-B/32 + scale-hyperprior compressor (the model behind the reference's headline table), MI355X kernels.

    state_dict   : what the reference's ``HRateHyperprior`` saves (``main.py`` training), as a dict or a path to it.  No
                   hyperprior checkpoint ships with the reference, so there is nothing to fetch:
                   ``lossyless_amd.HyperpriorFit(beta).fit(Z).state_dict()`` trains one on frozen features.
    coded_means  : ``"scales"`` (default; the reference's coder, which codes with the scales in the means' place) or
                   ``"predicted"`` (opt-in: code with the means the model was trained with -- a lower rate for a model of
                   one's own, not the reference's format).  The file does not record the mode: one written in one mode
                   and read in the other, like one read with another state dict, decodes to wrong values without an error.
    mlp_precision : ``"fp32"`` (default: the hyperprior MLPs on the fp32 matrix cores; files are decoded on the GPU only) or
                   ``"ordered"`` (opt-in: every MLP output one ascending ``fmaf`` chain, which the host reproduces bit for
                   bit -- ``decompress_dataset(file, is_cpu=True)`` then decodes without a GPU, also on a compressor built
                   with ``device="cpu"``).  Not recorded in the file either, with the same consequence.
    device, clip_weights, gpu_preprocess, other kwargs : as for ``clip_compressor_b005``; forwarded to
                   ``lossyless_amd.HyperpriorClipCompressor``

    Returns ``(compressor, transform)`` with the factorized entry points' surface; ``compress`` returns
    ``[z_strings, side_z_strings]``, the ``.bin`` file holds two records per image, and ``decompress_dataset`` decodes on
    the GPU (``is_cpu=True`` raises unless ``mlp_precision="ordered"``: the coding-table rows come from an MLP evaluated on
    the fp32 matrix cores).
    """
    model = _HyperpriorCompressor(pretrained_state_dict=state_dict, device=device, coded_means=coded_means,
                                  mlp_precision=mlp_precision, **kwargs)
    return model, model.preprocess


def clip_compressor(state_dict, device=_ON, **kwargs):
    """CLIP ViT-B/32 + entropy bottleneck compressor at a rate point of the caller's: the factorized sibling of
    ``clip_hyperprior_compressor``.

    state_dict   : what the reference's ``HRateFactorizedPrior`` saves -- ``lossyless_amd.BottleneckFit(beta).fit(Z)
                   .state_dict()``, or a ``main.py`` checkpoint's rate estimator -- as a dict or a path to it (the key set of
                   the shipped ``lossyless_amd/assets/*_factorized_rate.pt``).
    device, clip_weights, gpu_preprocess, other kwargs : as for ``clip_compressor_b005``; forwarded to
                   ``lossyless_amd.ClipCompressor``

    Returns ``(compressor, transform)`` with the surface of the three shipped rate points.
    """
    model = _Compressor(pretrained_state_dict=state_dict, device=device, **kwargs)
    return model, model.preprocess


def feature_compressor(state_dict, device=_ON):
    """Entropy-bottleneck compressor for FEATURES of any frozen encoder, at any width: ``clip_compressor`` without the tower
    and without CLIP weights.

    state_dict   : a factorized rate point -- ``lossyless_amd.BottleneckFit(beta).fit(Z).state_dict()`` on the features to
                   compress, or the reference's ``HRateFactorizedPrior`` -- as a dict or a path to it.  ``z_dim`` is read
                   from it (1024 for the RN50 CLIP tower, 2048 for the reference's SimCLR / SwAV ResNets, ...).
    device       : "cuda", or "cpu" for the library's host coder (same bytes, same values)

    Returns the compressor alone (there are no images, hence no transform): ``compressor(Z)`` -> reconstructed rows,
    ``compress`` / ``decompress`` / ``get_rate``, ``compress_dataset(Z, file, label_file=None, labels=None)`` with ``Z`` a
    ``[N, z_dim]`` tensor or an iterable of batches, ``decompress_dataset`` and ``open_dataset`` (the reference's ``.bin``
    format; at 512 dimensions the file ``clip_compressor`` writes for the same embeddings).
    """
    return _FeatureCompressor(pretrained_state_dict=state_dict, device=device)


def clip_text_encoder(clip_weights=None, device=_ON, **kwargs):
    """CLIP's text tower (``model.encode_text``), MI355X kernels: ``encoder(tokens [P, T]) -> [P, embed_dim]``, and
    ``encoder.encode_classes(tokens [K, n_templates, T])`` for ``lossyless_amd.ZeroShotProbe``.

    clip_weights : path to OpenAI ViT-B-32.pt (the file the compressors read: it holds both towers) / a state-dict; default
                   $LOSSYLESS_CLIP_WEIGHTS; "synthetic" = seed-1 random weights, tests and the bench tool only
    device       : "cuda", or "cpu" for the float64 twin
    other kwargs : forwarded to ``lossyless_amd.clip_text.TextTransformer`` (``chunk``, ``truncate``, ``tokenizer``)

    Tokens are integers; strings need ``tokenizer=`` (no vocabulary ships here).
    """
    from lossyless_amd.clip_text import TextTransformer, resolve_clip_text_weights
    return TextTransformer(resolve_clip_text_weights(clip_weights)[0], device=device, **kwargs)
