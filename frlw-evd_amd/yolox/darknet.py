"""The two backbones of the shipped recipes (reference: core/yolox/models/darknet.py).

``CSPDarknet`` (:270-354; built at core/exp.py:582 as ``CSPDarknet(C, 0.33, 0.5, stem=Focus)``) carries the ``yolox`` recipes,
``Darknet`` (:14-117; built at core/exp.py:369 as ``Darknet(21, img_size, stem, in_channels=C, out_channels=[256, 256, 256],
stem_out_channels=64)``) the paper's own AED detector of the ``basic`` / ``taf`` / ``taf_bfm`` recipes."""
import torch.nn as nn

from .network_blocks import BaseConv, CSPLayer, Focus, ResLayer, SPPBottleneck


class Darknet(nn.Module):
    """Darknet-21 with the reference's constructor signature and submodule names, so checkpoints interchange: stem, then per
    stage a 3x3 stride-2 BaseConv and 1, 2, 2, 1 ``ResLayer``s, and the five-layer SPP block behind ``dark5``."""
    depth2blocks = {21: [1, 2, 2, 1]}

    def __init__(self, depth, shape, stem=Focus, in_channels=3, stem_out_channels=64, out_channels=(256, 512, 1024),
                 out_features=("dark3", "dark4", "dark5"), act="silu"):
        super().__init__()
        assert out_features, "please provide output features of Darknet"
        if depth not in self.depth2blocks:
            raise NotImplementedError(f"Darknet-{depth}: the shipped recipes build depth 21 only (SURVEY.md section 8)")
        self.out_features = out_features
        self.stem = stem(in_channels, stem_out_channels, ksize=3, act=act)
        base = stem_out_channels
        n = self.depth2blocks[depth]
        self.dark2 = nn.Sequential(*self.make_group_layer(base, base * 2, n[0], 2, act=act))
        self.dark3 = nn.Sequential(*self.make_group_layer(base * 2, out_channels[0], n[1], 2, act=act))
        self.dark4 = nn.Sequential(*self.make_group_layer(out_channels[0], out_channels[1], n[2], 2, act=act))
        self.dark5 = nn.Sequential(*self.make_group_layer(out_channels[1], out_channels[2], n[3], 2, act=act),
                                   *self.make_spp_block([out_channels[2], out_channels[2]], base * 4, act=act))
        self.shape = shape

    @staticmethod
    def make_group_layer(in_channels, out_channels, num_blocks, stride, act="silu"):
        """A stride-`stride` 3x3 BaseConv, then `num_blocks` ResLayers."""
        return [BaseConv(in_channels, out_channels, 3, stride, act=act)] + [ResLayer(out_channels, act=act) for _ in range(num_blocks)]

    @staticmethod
    def make_spp_block(filters_list, in_filters, act="silu"):
        return nn.Sequential(BaseConv(in_filters, filters_list[0], 1, 1, act=act),
                             BaseConv(filters_list[0], filters_list[1], 3, 1, act=act),
                             SPPBottleneck(filters_list[1], filters_list[0], activation=act),
                             BaseConv(filters_list[0], filters_list[1], 3, 1, act=act),
                             BaseConv(filters_list[1], filters_list[0], 1, 1, act=act))

    def forward(self, x):
        outputs = {}
        x = self.stem(x)
        outputs["stem"] = x
        for name in ("dark2", "dark3", "dark4", "dark5"):
            x = getattr(self, name)(x)
            outputs[name] = x
        return [outputs[k] for k in self.out_features]


class CSPDarknet(nn.Module):
    def __init__(self, in_channel, dep_mul, wid_mul, out_features=("dark3", "dark4", "dark5"), depthwise=False,
                 act="silu", stem=Focus):
        super().__init__()
        assert out_features, "please provide output features of Darknet"
        if depthwise:
            raise NotImplementedError("depthwise convolutions are outside the hot path (SURVEY.md section 8)")
        self.out_features = out_features
        c = int(wid_mul * 64)
        d = max(round(dep_mul * 3), 1)
        self.stem = stem(in_channel, c, ksize=3, act=act)
        self.dark2 = nn.Sequential(BaseConv(c, c * 2, 3, 2, act=act),
                                   CSPLayer(c * 2, c * 2, n=d, depthwise=depthwise, act=act))
        self.dark3 = nn.Sequential(BaseConv(c * 2, c * 4, 3, 2, act=act),
                                   CSPLayer(c * 4, c * 4, n=d * 3, depthwise=depthwise, act=act))
        self.dark4 = nn.Sequential(BaseConv(c * 4, c * 8, 3, 2, act=act),
                                   CSPLayer(c * 8, c * 8, n=d * 3, depthwise=depthwise, act=act))
        self.dark5 = nn.Sequential(BaseConv(c * 8, c * 16, 3, 2, act=act),
                                   SPPBottleneck(c * 16, c * 16, activation=act),
                                   CSPLayer(c * 16, c * 16, n=d, shortcut=False, depthwise=depthwise, act=act))

    def forward(self, x):
        outputs = {}
        x = self.stem(x)
        outputs["stem"] = x
        for name in ("dark2", "dark3", "dark4", "dark5"):
            x = getattr(self, name)(x)
            outputs[name] = x
        return [outputs[k] for k in self.out_features]
