"""Generators resolvable by name, as src.model.nets is in the reference
(main.py:56 `_get_instance(src.model.nets, config.net)`)."""
from .base_net import BaseNet
from .bicubic import Bicubic
from .drf_net import DRFNet, DRFSISRNet
from .duf_net import DUFNet
from .edsr_net import EDSRNet
from .edvr_net import EDVRNet
from .frvsr_net import FRVSRNet
from .rbp_net import RBPNet
from .srfb_net import SRFBNet

__all__ = ["BaseNet", "EDSRNet", "DUFNet", "DRFNet", "DRFSISRNet", "SRFBNet", "Bicubic", "FRVSRNet", "EDVRNet",
           "RBPNet"]
