"""Eager PyTorch (MIOpen / hipBLASLt) forward of the ResNet-50 trunk for the yardstick tools ONLY: the package's modules have no eager route
(ResNet50Features.forward is the HIP path).  Works on the package's parameter containers."""
import torch
import torch.nn.functional as F


def _bn(x, bn):
    return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)


def _conv(x, c):
    return F.conv2d(x, c.weight, None, c.stride, c.padding)


def resnet50_eager(net, x):
    x = F.max_pool2d(F.relu(_bn(_conv(x, net.conv1), net.bn1)), 3, stride=2, padding=1)
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for b in layer:
            y = F.relu(_bn(_conv(x, b.conv1), b.bn1))
            y = F.relu(_bn(_conv(y, b.conv2), b.bn2))
            y = _bn(_conv(y, b.conv3), b.bn3)
            s = x if b.downsample is None else _bn(_conv(x, b.downsample[0]), b.downsample[1])
            x = F.relu(y + s)
    return x.mean(dim=(2, 3))


def resnet_pointnet_eager(net, p):
    """respointnet.py:33-59 on the package's ResnetPointnet parameter container: eager float32 ops, differentiable through torch's own autograd."""
    x = F.linear(p, net.fc_pos_0.weight, net.fc_pos_0.bias)
    for i in range(4):
        b = getattr(net, f"block_{i}")
        if i:
            x = torch.cat([x, x.max(dim=1, keepdim=True)[0].expand(x.size())], dim=2)
        x = F.linear(F.relu(F.linear(F.relu(x), b.fc_0.weight, b.fc_0.bias)), b.fc_1.weight, b.fc_1.bias) + F.linear(x, b.shortcut.weight)
    return F.linear(F.relu(x.max(dim=1)[0]), net.fc_c.weight, net.fc_c.bias)


SMPL_TO_OPENPOSE = [24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34]


def val_losses_eager(t, weights, penetration=None):
    """The evaluation-branch formulas of EgoHMR.compute_loss (egohmr.py:307-449) as eager float32 torch ops on the tensors of EgoHMR.loss_inputs:
    the yardstick for tools/bench_losses.py (what the reference launches, ground-truth `where`-copies included) -> ([11] losses, visible joints)."""
    import torch
    B = t["pred_vertices"].shape[0]
    fem = t["gender"] == 1
    gt_v, gt_j = t["gt_vertices_male"].clone(), t["gt_joints_male"].clone()
    gt_v[fem], gt_j[fem] = t["gt_vertices_female"][fem], t["gt_joints_female"][fem]
    conf = t["keypoints_2d"][:, :, -1:].clone()
    conf[:, [1, 9, 12]] = 0
    kp2d = (conf * (t["pred_keypoints_2d_full"][:, SMPL_TO_OPENPOSE] - t["keypoints_2d"][:, :, :-1]).abs()).sum(dim=(1, 2)).mean()
    p3, g3 = t["pred_keypoints_3d"][:, :24], t["keypoints_3d"][:, :24]
    p3a, g3a = p3 - p3[:, [0]], g3 - g3[:, [0]]
    kp3d = (p3a - g3a).abs().sum(dim=(1, 2)).mean()
    kp3d_full = (t["pred_keypoints_3d_full"][:, :24] - t["keypoints_3d_full"][:, :24]).abs().sum(dim=(1, 2)).mean()
    v2v = ((t["pred_vertices"] - p3[:, [0]]) - (gt_v - gt_j[:, [0]])).abs().mean()
    p = gt_j[:, :24] / gt_j[:, :24, 2:3]
    u = t["focal"][:, None, 0] * p[..., 0] + t["center"][:, None, 0] * p[..., 2]
    v = t["focal"][:, None, 1] * p[..., 1] + t["center"][:, None, 1] * p[..., 2]
    mask = (u >= 0) * (u < 1920) * (v >= 0) * (v < 1080)
    vis = (torch.sqrt(((p3a - g3a) ** 2).sum(-1)) * mask).sum()
    betas = ((t["pred_betas"] - t["gt_betas"]) ** 2).sum() / B
    bp = ((t["pred_body_pose"].reshape(B, -1) - t["gt_body_pose"]) ** 2).sum() / B
    go = ((t["pred_global_orient"].reshape(B, -1) - t["gt_global_orient"]) ** 2).sum() / B
    x = t["pred_pose_6d"].reshape(-1, 3, 2)
    ortho = ((torch.matmul(x.permute(0, 2, 1), x) - torch.eye(2, device=x.device)[None]) ** 2).mean()
    pen = penetration.mean() if penetration is not None else torch.zeros((), device=x.device)
    terms = [v2v, kp3d, kp3d_full, kp2d, betas, bp, go, ortho, pen]
    loss = sum(w * s for w, s in zip(weights, terms))
    return torch.stack([loss, *terms, vis]), mask.sum()
