"""A ResNet in eval mode as a float64 functional evaluation driven by a ``state_dict`` in torchvision's key layout alone
(``conv1``, ``bn1``, ``layer{i}.{j}.conv{k}`` / ``bn{k}`` / ``downsample.{0,1}``): ``F.conv2d``, ``F.batch_norm`` on the
running statistics, ``F.max_pool2d``.  It is written from the key layout and does not call any module's ``forward``: the
block kind follows from the presence of ``conv3``, the widths from the weights, and only the strides — which a
``state_dict`` does not hold — are arguments.
"""
import torch
import torch.nn.functional as F


def _bn(x, sd, name, eps):
    return F.batch_norm(x, sd[name + '.running_mean'], sd[name + '.running_var'], sd[name + '.weight'],
                        sd[name + '.bias'], False, 0.0, eps)


def resnet_eval(state_dict, x, strides=(1, 2, 2, 2), style='pytorch', eps=1e-5):
    """The outputs of all stages for input ``x``; everything in float64."""
    sd = {k: v.detach().cpu().double() for k, v in state_dict.items() if v.dtype.is_floating_point}
    x = x.detach().cpu().double()
    x = F.relu(_bn(F.conv2d(x, sd['conv1.weight'], stride=2, padding=3), sd, 'bn1', eps))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    outs, i = [], 1
    while f'layer{i}.0.conv1.weight' in sd:
        j = 0
        while f'layer{i}.{j}.conv1.weight' in sd:
            p = f'layer{i}.{j}.'
            stride = strides[i - 1] if j == 0 else 1
            identity = x
            if p + 'downsample.0.weight' in sd:
                identity = _bn(F.conv2d(x, sd[p + 'downsample.0.weight'], stride=stride), sd, p + 'downsample.1', eps)
            if p + 'conv3.weight' in sd:           # bottleneck: 1 x 1, 3 x 3, 1 x 1
                s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
                y = F.relu(_bn(F.conv2d(x, sd[p + 'conv1.weight'], stride=s1), sd, p + 'bn1', eps))
                y = F.relu(_bn(F.conv2d(y, sd[p + 'conv2.weight'], stride=s2, padding=1), sd, p + 'bn2', eps))
                y = _bn(F.conv2d(y, sd[p + 'conv3.weight']), sd, p + 'bn3', eps)
            else:                                  # basic: 3 x 3, 3 x 3
                y = F.relu(_bn(F.conv2d(x, sd[p + 'conv1.weight'], stride=stride, padding=1), sd, p + 'bn1', eps))
                y = _bn(F.conv2d(y, sd[p + 'conv2.weight'], padding=1), sd, p + 'bn2', eps)
            x = F.relu(y + identity)
            j += 1
        outs.append(x)
        i += 1
    return outs
