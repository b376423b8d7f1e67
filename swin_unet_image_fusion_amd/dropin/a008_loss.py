"""Drop-in shim: put this directory on sys.path and the reference's import line
`from a008_loss import MyLoss` resolves to the HIP-backed implementation (settings are keyword arguments of MyLoss, with the
reference's A000_CONFIG values as defaults)."""
from swin_unet_image_fusion_amd.loss import MyLoss  # noqa: F401
