"""Networks of the learning baselines.  ``DenseActionSpaceDQN`` is the fully convolutional Q-network of the spatial-action-map baseline (SAM): one Q value
per pixel of the observation.  Written from its description; the parameter names are the reference's (benchpush/baselines/feature_extractors.py), so a
checkpoint trained there loads here with ``load_state_dict(strict=True)`` (tests/golden/sam_state_dict.json pins names, shapes and one float64 output).
"""
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["DenseActionSpaceDQN", "ResNet18NoNorm", "ResidualBlock"]


class ResidualBlock(nn.Module):
    """Two 3x3 convolutions without bias and without normalisation, ReLU between them, plus the input (through `downsample` where the width changes)."""

    def __init__(self, width_in, width, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(width_in, width, 3, padding=1, bias=False)
        self.conv2 = nn.Conv2d(width, width, 3, padding=1, bias=False)
        self.downsample = downsample

    def forward(self, x):
        skip = x if self.downsample is None else self.downsample(x)
        return F.relu(self.conv2(F.relu(self.conv1(x))) + skip)


class ResNet18NoNorm(nn.Module):
    """ResNet-18 trunk (four stages of two blocks, 64 -> 128 -> 256 -> 512) without batch norm: a 7x7 stride-2 stem, a 3x3 stride-2 max-pool, and every
    stage at stride 1, so the features are a quarter of the input's side.  Convolutions start from Kaiming-normal fan-out weights.  ``fc`` is the
    1000-way classifier of the stock model: ``features`` does not use it; it is kept because the reference's checkpoints carry its weights."""

    WIDTHS = (64, 128, 256, 512)

    def __init__(self, num_input_channels=3, num_classes=1000):
        super().__init__()
        self.conv1 = nn.Conv2d(num_input_channels, 64, 7, stride=2, padding=3, bias=False)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        width_in = 64
        for i, width in enumerate(self.WIDTHS):
            down = None if width == width_in else nn.Sequential(nn.Conv2d(width_in, width, 1, bias=False))
            setattr(self, "layer%d" % (i + 1), nn.Sequential(ResidualBlock(width_in, width, down), ResidualBlock(width, width)))
            width_in = width
        self.fc = nn.Linear(512, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def features(self, x):
        x = self.maxpool(F.relu(self.conv1(x)))
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))

    def forward(self, x):
        return self.fc(self.features(x).mean(dim=(2, 3)))


class DenseActionSpaceDQN(nn.Module):
    """[N, num_input_channels, P, P] -> [N, num_output_channels, P, P]: the trunk's [N, 512, P/4, P/4] features, then 1x1 convolutions 512 -> 128 -> 32 ->
    outputs with a ReLU and a x2 bilinear (align_corners) upsampling after each of the first two.  P must be a multiple of 4."""

    def __init__(self, num_input_channels=3, num_output_channels=1):
        super().__init__()
        self.resnet18 = ResNet18NoNorm(num_input_channels=num_input_channels)
        self.conv1 = nn.Conv2d(512, 128, 1)
        self.conv2 = nn.Conv2d(128, 32, 1)
        self.conv3 = nn.Conv2d(32, num_output_channels, 1)

    def forward(self, x):
        x = self.resnet18.features(x)
        for conv in (self.conv1, self.conv2):
            x = F.interpolate(F.relu(conv(x)), scale_factor=2, mode="bilinear", align_corners=True)
        return self.conv3(x)
