"""Plain torch.nn restatement of torchvision's DenseNet ``features`` (Huang et al., densely connected convolutional networks), written from the
published architecture with torchvision's key names: conv0, norm0, denseblockK.denselayerL.{norm1,conv1,norm2,conv2}, transitionK.{norm,conv},
norm5; kaiming-normal convolutions, BatchNorm 1 / 0.  The reference the DenseNet encoder tests compare against (helper, no tests)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class DenseLayer(nn.Module):
    def __init__(self, cin, growth, bn_size):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, bn_size * growth, 1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth)
        self.conv2 = nn.Conv2d(bn_size * growth, growth, 3, 1, 1, bias=False)

    def forward(self, feats):
        y = self.conv1(F.relu(self.norm1(torch.cat(feats, 1))))
        return self.conv2(F.relu(self.norm2(y)))


class DenseBlock(nn.Module):
    def __init__(self, n, cin, growth, bn_size):
        super().__init__()
        for i in range(n):
            self.add_module(f"denselayer{i + 1}", DenseLayer(cin + i * growth, growth, bn_size))

    def forward(self, x):
        feats = [x]
        for layer in self.children():
            feats.append(layer(feats))
        return torch.cat(feats, 1)


class Transition(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm = nn.BatchNorm2d(cin)
        self.conv = nn.Conv2d(cin, cout, 1, bias=False)

    def forward(self, x):
        return F.avg_pool2d(self.conv(F.relu(self.norm(x))), 2, 2)


class DenseNetFeatures(nn.Module):
    def __init__(self, growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4):
        super().__init__()
        self.conv0 = nn.Conv2d(3, num_init_features, 7, 2, 3, bias=False)
        self.norm0 = nn.BatchNorm2d(num_init_features)
        nf = num_init_features
        self.nblocks = len(block_config)
        for i, n in enumerate(block_config):
            self.add_module(f"denseblock{i + 1}", DenseBlock(n, nf, growth_rate, bn_size))
            nf += n * growth_rate
            if i + 1 < len(block_config):
                self.add_module(f"transition{i + 1}", Transition(nf, nf // 2))
                nf //= 2
        self.norm5 = nn.BatchNorm2d(nf)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)

    def features(self, x):
        """The five maps the BTS encoder returns: relu0, pool0, transition1, transition2, relu(norm5) (NCHW)."""
        f0 = F.relu(self.norm0(self.conv0(x)))
        x = F.max_pool2d(f0, 3, 2, 1)
        out = [f0, x]
        for i in range(1, self.nblocks):
            x = getattr(self, f"transition{i}")(getattr(self, f"denseblock{i}")(x))
            out.append(x)
        x = F.relu(self.norm5(getattr(self, f"denseblock{self.nblocks}")(x)))
        return out[:4] + [x]


def densenet121():
    return DenseNetFeatures(32, (6, 12, 24, 16), 64)


def densenet161():
    return DenseNetFeatures(48, (6, 12, 36, 24), 96)
