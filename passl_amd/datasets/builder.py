"""DATASETS registry + build_dataloader (reference passl_v110/datasets/builder.py:25-105).

Only the synthetic two-view source is built: the benchmark and the parity tests use synthetic
tensors, and the reference's PIL/cv2 augmentation pipeline is outside the accelerated path
(SURVEY §2.1 row 9).  ``name: ImageNet`` from the reference configs resolves to a class that
explains this instead of silently substituting data."""
from ..utils.registry import Registry, build_from_config

DATASETS = Registry('DATASET')


def build_dataset(cfg):
    return build_from_config(cfg, DATASETS)


def build_dataloader(cfg, device):
    """cfg = dataloader.train block: {loader, sampler, dataset}.  Returns (loader, mixup_fn): ``dataset.batch_transforms``
    is popped as the reference does (builder.py:88-103) and built by preprocess.build_mixup — a Mixup when the block
    mixes, else None.  The Trainer hands it to every model call; only the train block's is used.
    A ``RandomErasing`` entry of ``dataset.transforms`` (preprocess.build_random_erasing) of a SyntheticLabeled source
    becomes the loader's ``batch_transform``: erasing happens in the loader, i.e. before ``mixup_fn`` — the reference's
    order, per-sample transform first, then the collate-time mix.  Every other entry stays ignored there.
    A SyntheticRawLabeled source (uint8 HWC images) honours its whole ``transforms`` list: crop, flip, NormalizeImage and
    ToCHWImage become one preprocess.DeviceCropPipeline, followed by the eraser when the list ends in ``RandomErasing``.
    A SyntheticRawTwoView source honours its ``transform`` block (the v2 schema's key; ``transforms`` is read too): one
    TwoViewsTransform of two view pipelines (preprocess.view_aug), so the loader yields (x_q, x_k) of the same images."""
    from .preprocess import build_mixup, build_random_erasing
    from .preprocess.crop import ChainedBatchTransform, build_crop_pipeline
    from .synthetic import SyntheticLabeled, SyntheticLoader, SyntheticRawLabeled, SyntheticRawTwoView
    ds_cfg = dict(cfg['dataset'])
    mixup_cfg = ds_cfg.pop('batch_transforms', None)
    sampler = cfg.get('sampler', {})
    dataset = build_dataset(ds_cfg)
    eraser = build_random_erasing(ds_cfg.get('transforms', None)) if isinstance(dataset, SyntheticLabeled) else None
    if isinstance(dataset, SyntheticRawLabeled):
        crop = build_crop_pipeline(ds_cfg.get('transforms', None))
        eraser = crop if eraser is None else ChainedBatchTransform([crop, eraser])
    if isinstance(dataset, SyntheticRawTwoView):
        from .preprocess.view_aug import build_two_views
        eraser = build_two_views(ds_cfg.get('transform', None) or ds_cfg.get('transforms', None))
    loader = SyntheticLoader(dataset, batch_size=sampler.get('batch_size', 32), device=device,
                             drop_last=sampler.get('drop_last', True), batch_transform=eraser)
    ring = int((cfg.get('loader', None) or {}).get('host_ring', 0) or 0)
    if ring:
        from .synthetic import HostRingLoader
        loader = HostRingLoader(loader, ring=ring)       # batches move host -> device one step ahead of the step
    return loader, build_mixup(mixup_cfg)
