"""Networks of the learning baselines.  ``DenseActionSpaceDQN`` is the fully convolutional Q-network of the spatial-action-map baseline (SAM): one Q value
per pixel of the observation.  Written from its description; the parameter names are the reference's (benchpush/baselines/feature_extractors.py), so a
checkpoint trained there loads here with ``load_state_dict(strict=True)`` (tests/golden/sam_state_dict.json pins names, shapes and one float64 output).

``ResNet18Extractor`` and ``ActorCriticCnn`` are the networks of the PPO baselines (benchpush_amd/baselines/ppo.py).  The reference builds them from
torchvision's ``resnet18`` and stable-baselines3's ``ActorCriticCnnPolicy``; neither package is available to this project's build, so the parameter
names below are argued from the documented structure of the two and are not pinned by a fixture of the reference.

``SacActor``, ``SacCritic`` and ``SacPolicy`` are the networks of the SAC baselines (benchpush_amd/baselines/sac.py), laid out as stable-baselines3's SAC
``CnnPolicy`` names its parts, under the same caveat.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["ActorCriticCnn", "BasicBlockBN", "DenseActionSpaceDQN", "ResNet18Extractor", "ResNet18NoNorm", "ResidualBlock", "SacActor", "SacCritic",
           "SacPolicy", "squashed_gaussian_log_prob"]


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


class BasicBlockBN(nn.Module):
    """The stock ResNet basic block: 3x3 convolution (stride `stride`), batch norm, ReLU, 3x3 convolution, batch norm, plus the input (through
    `downsample`, a 1x1 stride-`stride` convolution with batch norm, where the shape changes), ReLU."""

    def __init__(self, width_in, width, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(width_in, width, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(width, width, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.downsample = None
        if stride != 1 or width_in != width:
            self.downsample = nn.Sequential(nn.Conv2d(width_in, width, 1, stride=stride, bias=False), nn.BatchNorm2d(width))

    def forward(self, x):
        skip = x if self.downsample is None else self.downsample(x)
        return self.relu(self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x))))) + skip)


class ResNet18Extractor(nn.Module):
    """[N, C, H, W] -> [N, 512]: the stock ResNet-18 with batch norm and stride-2 stages, a stem for the env's channel count (7x7 stride-2 convolution
    without bias, like the stock stem it replaces), global average pooling instead of the classifier.  ``resnet`` is an
    ``nn.Sequential`` whose children stand in the stock model's order -- 0 stem convolution, 1 its batch norm, 2 ReLU, 3 max-pool, 4 .. 7 the stages, 8
    the average pool -- so the parameters are called ``resnet.0.weight``, ``resnet.1.running_mean``, ``resnet.4.0.conv1.weight``,
    ``resnet.5.0.downsample.0.weight`` and so on."""

    WIDTHS = (64, 128, 256, 512)

    def __init__(self, num_input_channels=4, features_dim=512):
        super().__init__()
        if features_dim != 512:
            raise ValueError("ResNet18Extractor: the trunk gives 512 features")
        self.features_dim = 512
        layers = [nn.Conv2d(num_input_channels, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(3, stride=2, padding=1)]
        width_in = 64
        for i, width in enumerate(self.WIDTHS):
            layers.append(nn.Sequential(BasicBlockBN(width_in, width, stride=1 if i == 0 else 2), BasicBlockBN(width, width)))
            width_in = width
        layers.append(nn.AdaptiveAvgPool2d((1, 1)))
        self.resnet = nn.Sequential(*layers)

    def forward(self, x):
        return torch.flatten(self.resnet(x), 1)


class _MlpExtractor(nn.Module):
    def __init__(self, features_dim, pi, vf):
        super().__init__()

        def net(widths):
            layers, w_in = [], features_dim
            for w in widths:
                layers += [nn.Linear(w_in, w), nn.Tanh()]
                w_in = w
            return nn.Sequential(*layers)
        self.policy_net, self.value_net = net(pi), net(vf)
        self.latent_dim_pi, self.latent_dim_vf = pi[-1], vf[-1]


class ActorCriticCnn(nn.Module):
    """Gaussian actor-critic on image observations, laid out as stable-baselines3's ``ActorCriticCnnPolicy`` with the reference's arguments
    (features_extractor_class ResNet18, net_arch pi = vf = [512, 256]): ``features_extractor`` (shared by actor and critic),
    ``mlp_extractor.policy_net`` and ``mlp_extractor.value_net`` (512 -> 512 -> 256 with tanh: Linear layers 0 and 2 of each), ``action_net``
    (256 -> action_dim, the mean), ``value_net`` (256 -> 1) and a state-independent ``log_std`` (zeros).  Linear and convolution weights start
    orthogonal with gain sqrt(2) (``action_net`` 0.01, ``value_net`` 1) and zero bias, as that policy's ``ortho_init`` does.  stable-baselines3 2.x
    also registers the shared extractor as ``pi_features_extractor`` and ``vf_features_extractor``; a checkpoint of its policy carries those duplicate
    keys, which ``load_state_dict(strict=False)`` skips.  Observations are float [N, C, H, W] in [0, 1] (uint8 / 255)."""

    def __init__(self, num_input_channels=4, action_dim=1, net_arch=None):
        super().__init__()
        arch = net_arch or dict(pi=[512, 256], vf=[512, 256])
        self.action_dim = int(action_dim)
        self.features_extractor = ResNet18Extractor(num_input_channels)
        self.mlp_extractor = _MlpExtractor(512, list(arch["pi"]), list(arch["vf"]))
        self.action_net = nn.Linear(self.mlp_extractor.latent_dim_pi, self.action_dim)
        self.value_net = nn.Linear(self.mlp_extractor.latent_dim_vf, 1)
        self.log_std = nn.Parameter(torch.zeros(self.action_dim))
        for module, gain in ((self.features_extractor, math.sqrt(2)), (self.mlp_extractor, math.sqrt(2)), (self.action_net, 0.01), (self.value_net, 1.0)):
            for m in module.modules():
                if isinstance(m, (nn.Linear, nn.Conv2d)):
                    nn.init.orthogonal_(m.weight, gain=gain)
                    if m.bias is not None:
                        m.bias.data.fill_(0.0)

    def forward(self, obs):
        """(mean [N, A], value [N])."""
        f = self.features_extractor(obs)
        return self.action_net(self.mlp_extractor.policy_net(f)), self.value_net(self.mlp_extractor.value_net(f)).squeeze(1)

    def value(self, obs):
        return self.value_net(self.mlp_extractor.value_net(self.features_extractor(obs))).squeeze(1)

    def log_prob(self, mean, actions):
        """log N(actions; mean, exp(log_std)) summed over the action columns, [N]."""
        var = torch.exp(2.0 * self.log_std)
        return (-((actions - mean) ** 2) / (2.0 * var) - self.log_std - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)


LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0      # stable-baselines3's clamp of the SAC actor's log_std
SQUASH_EPS = 1e-6                          # its epsilon inside the log of the tanh correction


def squashed_gaussian_log_prob(mean, log_std, gaussian_actions):
    """log-density [N] of ``tanh(gaussian_actions)`` for ``gaussian_actions ~ N(mean, exp(log_std))``: the Gaussian's log-density summed over the
    action columns minus ``sum log(1 - tanh(u)^2 + 1e-6)``, as stable-baselines3's SquashedDiagGaussianDistribution computes it."""
    normal = -((gaussian_actions - mean) ** 2) / (2.0 * torch.exp(2.0 * log_std)) - log_std - 0.5 * math.log(2.0 * math.pi)
    return normal.sum(dim=1) - torch.log(1.0 - torch.tanh(gaussian_actions) ** 2 + SQUASH_EPS).sum(dim=1)


def _relu_mlp(w_in, widths, w_out=None):
    layers = []
    for w in widths:
        layers += [nn.Linear(w_in, w), nn.ReLU()]
        w_in = w
    if w_out is not None:
        layers.append(nn.Linear(w_in, w_out))
    return nn.Sequential(*layers)


class SacActor(nn.Module):
    """The actor of stable-baselines3's SAC ``CnnPolicy`` with the reference's arguments: ``features_extractor`` (ResNet18, 512 features), ``latent_pi``
    (512 -> 512 -> 256 with ReLU: Linear layers 0 and 2), ``mu`` and a state-dependent ``log_std`` (256 -> action_dim each), the latter clamped to
    [-20, 2].  `features_extractor` and `net_arch` can be replaced (the CPU tests use a small flat extractor)."""

    def __init__(self, num_input_channels=4, action_dim=1, net_arch=(512, 256), features_extractor=None, features_dim=512):
        super().__init__()
        self.action_dim = int(action_dim)
        self.features_extractor = features_extractor if features_extractor is not None else ResNet18Extractor(num_input_channels)
        self.latent_pi = _relu_mlp(features_dim, list(net_arch))
        self.mu = nn.Linear(net_arch[-1], self.action_dim)
        self.log_std = nn.Linear(net_arch[-1], self.action_dim)

    def forward(self, obs):
        """(mean [N, A], log_std [N, A] clamped)."""
        latent = self.latent_pi(self.features_extractor(obs))
        return self.mu(latent), torch.clamp(self.log_std(latent), LOG_STD_MIN, LOG_STD_MAX)

    def action_log_prob(self, obs, noise=None, generator=None):
        """A sampled action ``tanh(mean + exp(log_std) * noise)`` [N, A] and its log-probability [N]; `noise` standard normal [N, A] (drawn from
        `generator` where None)."""
        mean, log_std = self(obs)
        if noise is None:
            noise = torch.randn(mean.shape, dtype=mean.dtype, device=mean.device, generator=generator)
        u = mean + torch.exp(log_std) * noise
        return torch.tanh(u), squashed_gaussian_log_prob(mean, log_std, u)

    def deterministic(self, obs):
        """tanh(mean) [N, A]."""
        return torch.tanh(self(obs)[0])


class SacCritic(nn.Module):
    """The critic of stable-baselines3's SAC ``CnnPolicy`` (``share_features_extractor=False``): its own ``features_extractor`` and two Q networks
    ``qf0``, ``qf1``, each (features + action_dim) -> 512 -> 256 -> 1 with ReLU (Linear layers 0, 2 and 4)."""

    def __init__(self, num_input_channels=4, action_dim=1, net_arch=(512, 256), features_extractor=None, features_dim=512):
        super().__init__()
        self.features_extractor = features_extractor if features_extractor is not None else ResNet18Extractor(num_input_channels)
        self.qf0 = _relu_mlp(features_dim + int(action_dim), list(net_arch), 1)
        self.qf1 = _relu_mlp(features_dim + int(action_dim), list(net_arch), 1)

    def forward(self, obs, actions):
        """(Q0 [N, 1], Q1 [N, 1])."""
        x = torch.cat([self.features_extractor(obs), actions], dim=1)
        return self.qf0(x), self.qf1(x)


class SacPolicy(nn.Module):
    """``actor``, ``critic`` and ``critic_target`` (a copy of the critic that takes no gradient and stays in eval mode), the names of stable-baselines3
    2.x's SAC policy.  Linear and convolution layers keep torch's default initialisation, as that policy does.  Like the PPO names above, these are argued
    from the documented structure of the package and are not pinned against it.  `make_extractor`: a callable that returns a fresh extractor with
    `features_dim` outputs (default: ResNet18Extractor(num_input_channels))."""

    def __init__(self, num_input_channels=4, action_dim=1, net_arch=(512, 256), make_extractor=None, features_dim=512):
        super().__init__()
        fe = make_extractor if make_extractor is not None else (lambda: ResNet18Extractor(num_input_channels))
        self.actor = SacActor(num_input_channels, action_dim, net_arch, fe(), features_dim)
        self.critic = SacCritic(num_input_channels, action_dim, net_arch, fe(), features_dim)
        self.critic_target = SacCritic(num_input_channels, action_dim, net_arch, fe(), features_dim)
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.critic_target.requires_grad_(False)
        self.critic_target.eval()

    def train(self, mode=True):
        """Actor and critic follow `mode`; the target stays in eval mode (its batch-norm statistics are copies of the critic's)."""
        super().train(mode)
        self.critic_target.eval()
        return self
