"""pssr2_amd — MI355X-native hot path of PSSR2 (ResUNet train/infer, MS-SSIM+L1 loss, crappifiers)."""
__version__ = "0.1.0"

from .crappifiers import AdditiveGaussian, Blur, Crappifier, MultiCrappifier, Poisson, SaltPepper, ScanPhase  # noqa: E402,F401


def __getattr__(name):
    # torch-dependent symbols are imported lazily so that `import pssr2_amd` stays cheap
    if name in ("ResUNet",):
        from .models import ResUNet
        return ResUNet
    if name in ("RDResUNet",):
        from .models import RDResUNet
        return RDResUNet
    if name in ("ResUNetA", "RDResUNetA"):
        from . import models
        return getattr(models, name)
    if name in ("SwinIR",):
        from .swinir import SwinIR
        return SwinIR
    if name in ("SSIMLoss",):
        from .util import SSIMLoss
        return SSIMLoss
    if name in ("train_paired",):
        from .train import train_paired
        return train_paired
    if name in ("train_crappifier",):
        from .train import train_crappifier
        return train_crappifier
    if name in ("approximate_crappifier",):
        from .train import approximate_crappifier
        return approximate_crappifier
    if name in ("ArrayDataset", "ImageDataset", "DeviceTileDataset"):
        from . import data
        return getattr(data, name)
    if name in ("PairedArrayDataset", "PairedImageDataset", "DevicePairedTileDataset"):
        from . import data
        return getattr(data, name)
    if name in ("SlidingSheetDataset", "SlidingDataset", "PairedSlidingArrayDataset", "PairedSlidingDataset", "DeviceSlidingDataset",
                "DevicePairedSlidingDataset"):
        from . import data
        return getattr(data, name)
    if name in ("GradHist",):
        from .models import GradHist
        return GradHist
    if name in ("predict_images",):
        from .predict import predict_images
        return predict_images
    if name in ("predict_collage",):
        from .predict import predict_collage
        return predict_collage
    if name in ("preprocess_dataset",):
        from .data import preprocess_dataset
        return preprocess_dataset
    if name in ("frc",):
        from .util import frc
        return frc
    if name in ("decorr",):
        from .util import decorr
        return decorr
    if name in ("frc_sectors", "decorr_sectors"):
        from . import util
        return getattr(util, name)
    if name in ("estimate_rsf",):
        from .util import estimate_rsf
        return estimate_rsf
    if name in ("estimate_noise",):
        from .util import estimate_noise
        return estimate_noise
    if name in ("Baseline",):
        from .baselines import Baseline
        return Baseline
    if name in ("upsample", "nlm_denoise"):
        from . import util
        return getattr(util, name)
    if name in ("FusedAdamW",):
        from .optim import FusedAdamW
        return FusedAdamW
    raise AttributeError(name)
