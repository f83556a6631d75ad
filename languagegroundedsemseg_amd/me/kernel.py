"""RegionType / KernelGenerator -- the kernel-shape descriptors of the ME surface
(/root/reference/models/modules/common.py:55-64,192-193,219-226).  On D=3 the model family only
uses HYPER_CUBE regions; SUPPORTED_CONVS below is the one statement of the (kernel_size, stride, dilation) it may ask for."""
import collections
import collections.abc
from enum import Enum

import torch


# The convolutions a kernel map exists for: the relations of the engine's classifier (csrc/lgs_common.h, KmapRelation), the plain and the
# dilated 3^3 stride-1 map folded into one row.  `what` names the convolution where a backend that does not build its map refuses it.
ConvRelation = collections.namedtuple("ConvRelation", "name kernel_size stride any_dilation what")
SUPPORTED_CONVS = (
    ConvRelation("conv3", 3, 1, True, "a 3x3x3 convolution"),
    ConvRelation("conv3_s2", 3, 2, False, "a 3x3x3 stride-2 convolution"),
    ConvRelation("conv2_s2", 2, 2, False, "a 2x2x2 stride-2 convolution"),
    ConvRelation("identity", 1, 1, False, "a 1x1 convolution"),
    ConvRelation("conv1_s2", 1, 2, False, "a 1x1 stride-2 convolution"),
)
CONV3_DILATED = SUPPORTED_CONVS[0]._replace(name="conv3_dilated", what="a dilated convolution")   # conv3 with dilation >= 2
ALL_CONV_RELATIONS = tuple(r.name for r in SUPPORTED_CONVS) + (CONV3_DILATED.name,)
# what a pair search between two coordinate sets builds: any dilation-1 map (its 1x1 map is the identity: no stride-2 form)
GENERIC_CONV_RELATIONS = ("identity", "conv3", "conv2_s2", "conv3_s2")


def conv_relation(kernel_size, stride, dilation):
    """-> the ConvRelation of an isotropic (kernel_size, stride, dilation), or None outside the supported set"""
    for r in SUPPORTED_CONVS:
        if (r.kernel_size, r.stride) == (kernel_size, stride) and (dilation == 1 or (r.any_dilation and dilation > 1)):
            return CONV3_DILATED if dilation > 1 else r
    return None


def supported_convs_text():
    """"(3, 1, d >= 1), (3, 2, 1), ... and (1, 2, 1)": the supported set as the refusal of an unsupported convolution lists it"""
    rows = ["(%d, %d, %s)" % (r.kernel_size, r.stride, "d >= 1" if r.any_dilation else "1") for r in SUPPORTED_CONVS]
    return ", ".join(rows[:-1]) + " and " + rows[-1]


class RegionType(Enum):
    HYPER_CUBE = 0
    HYPER_CROSS = 1
    CUSTOM = 2


def convert_to_int_list(arg, dimension):
    if isinstance(arg, torch.Tensor):
        arg = arg.tolist()
    if isinstance(arg, collections.abc.Sequence):
        assert len(arg) == dimension, "argument length %d != dimension %d" % (len(arg), dimension)
        return [int(a) for a in arg]
    return [int(arg)] * dimension


def convert_to_int_tensor(arg, dimension):
    return torch.IntTensor(convert_to_int_list(arg, dimension))


def convert_region_type(region_type, tensor_stride=None, kernel_size=None, up_stride=None, dilation=None,
                        region_offset=None, axis_types=None, dimension=None, center=True):
    """Kept for import compatibility (models/conditional_random_fields.py:5-6)."""
    return region_type, region_offset, 0


def get_kernel_volume(region_type, kernel_size, region_offset=None, axis_types=None, dimension=3):
    ks = convert_to_int_list(kernel_size, dimension)
    if region_type == RegionType.HYPER_CUBE:
        v = 1
        for k in ks:
            v *= k
        return v
    if region_type == RegionType.HYPER_CROSS:
        return sum(k - 1 for k in ks) + 1
    return int(region_offset.shape[0]) if region_offset is not None else 0


class KernelGenerator:
    def __init__(self, kernel_size=-1, stride=1, dilation=1, is_transpose=False, region_type=RegionType.HYPER_CUBE,
                 region_offsets=None, expand_coordinates=False, axis_types=None, dimension=-1):
        assert dimension > 0
        self.dimension = dimension
        self.kernel_size = convert_to_int_list(kernel_size, dimension)
        self.kernel_stride = convert_to_int_list(stride, dimension)
        self.kernel_dilation = convert_to_int_list(dilation, dimension)
        self.region_type = region_type if region_type is not None else RegionType.HYPER_CUBE
        self.region_offsets = region_offsets
        self.axis_types = axis_types
        self.is_transpose = is_transpose
        self.expand_coordinates = expand_coordinates
        self.kernel_volume = get_kernel_volume(self.region_type, self.kernel_size, region_offsets, axis_types, dimension)
