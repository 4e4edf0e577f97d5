"""CPU: the float64 batched proxy (oracle.collision.exact_proxy), the reference of tests/test_gpu_collision.py, pinned to the per-item
autograd proxy (proxy_collision_loss) and the occupancy stand-in (proxy_occupancy) it restates."""
import numpy as np
import torch

from oracle.collision import TAU, exact_proxy, proxy_collision_loss, proxy_occupancy


def _case(seed, B=3, V=300, N=700):
    g = np.random.Generator(np.random.PCG64(seed))
    verts = torch.from_numpy(g.uniform(-0.3, 0.3, size=(B, V, 3)))
    near = verts[:, g.integers(0, V, size=N // 2)] + torch.from_numpy(g.normal(scale=0.03, size=(B, N // 2, 3)))
    scene = torch.cat([near, torch.from_numpy(g.uniform(-0.5, 0.5, size=(B, N - N // 2, 3)))], dim=1)
    return verts, scene


def _per_item(verts, scene, all_points):
    loss, grad, occ = [], [], []
    for b in range(verts.shape[0]):
        v = verts[[b]].clone().requires_grad_()
        pts = scene[[b]]
        if not all_points:
            pts = pts[((pts >= v.min(1).values.detach()) & (pts <= v.max(1).values.detach())).all(-1)].unsqueeze(0)
        l = proxy_collision_loss(pts, v)
        l.backward()
        loss.append(l.detach())
        grad.append(v.grad[0])
        occ.append(proxy_occupancy(pts, v.detach()).sum())
    return torch.stack(loss), torch.stack(grad), torch.stack(occ)


def test_exact_proxy_matches_the_per_item_proxy():
    for seed, all_points in ((1, False), (2, True), (3, False)):
        verts, scene = _case(seed)
        r = exact_proxy(verts, scene, all_points=all_points)
        loss, grad, occ = _per_item(verts, scene, all_points)
        assert float(loss.min()) > 0
        torch.testing.assert_close(r["loss"], loss, rtol=1e-12, atol=1e-15)
        torch.testing.assert_close(r["gverts"], grad, rtol=1e-10, atol=1e-14)
        assert torch.equal(r["hits"], occ.long())
        # the selection is the bounding box, faces included
        if not all_points:
            lo, hi = verts.min(1, keepdim=True).values, verts.max(1, keepdim=True).values
            assert torch.equal(r["selected"], ((scene >= lo) & (scene <= hi)).all(-1))
        assert int(r["ncontrib"].sum()) == int(r["hits"].sum())


def test_exact_proxy_ties_faces_and_coincident_points():
    verts, _ = _case(4, B=1, V=50)
    verts = torch.cat([verts, verts[:, :10]], dim=1)          # vertices 50..59 duplicate 0..9: exact ties
    lo, hi = verts.min(1).values[0], verts.max(1).values[0]
    v0, vhi, vlo = verts[0, 0], verts[0, int(verts[0, :, 0].argmax())], verts[0, int(verts[0, :, 0].argmin())]
    pts = [v0 + torch.tensor([0.01, 0.0, 0.0]),                # nearest: vertex 0 and its duplicate 50
           v0.clone(),                                         # a point on a vertex: finite, zero gradient for the pair
           torch.stack([hi[0], vhi[1] + 0.01, vhi[2]]),        # on the max-x face: selected
           torch.stack([lo[0] - 1e-3, vlo[1], vlo[2]])]        # just outside the min-x face: not selected
    scene = torch.stack(pts).unsqueeze(0)
    r = exact_proxy(verts, scene)
    assert r["selected"][0].tolist() == [True, True, True, False]
    assert int(r["nearest"][0, 0]) == 0 and int(r["nearest"][0, 1]) == 0
    assert float(r["gap"][0, 0]) > 0                           # the duplicate is not the second-nearest vertex
    assert torch.isfinite(r["gverts"]).all() and float(r["gverts"][0, 50:60].abs().max()) == 0.0
    assert abs(float(r["d"][0, 1]) - 1e-6) < 1e-12
    loss, grad, _ = _per_item(verts, scene, False)
    torch.testing.assert_close(r["loss"], loss, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(r["gverts"], grad, rtol=1e-10, atol=1e-14)
    # all points: the point outside the box is taken too
    r2 = exact_proxy(verts, scene, all_points=True)
    assert bool(r2["selected"].all()) and float(r2["loss"][0]) > float(r["loss"][0])
    assert TAU == 0.05
