"""CPU: what the slab scene of tests/test_render_skip_run_gpu.py puts in front of the skip marcher's run loop.
The C oracle's per-sample weights give the transmittance at every free-space sample (alpha is the constant alpha_free
there, so T = w / alpha_free); printed: how many rays carry a T in [1e-10, 2e-10] into further free samples, and on which
side of the run loop's 2e-10 guard the 8 x 8 ray tiles (one wavefront each) enter the free space behind the slab.
    python scripts/skip_run_slab_stats.py"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import oracle
from selfocc_amd.render import RenderConfig

spec = importlib.util.spec_from_file_location("skip_run_tests", os.path.join(ROOT, "tests", "test_render_skip_run_gpu.py"))
t = importlib.util.module_from_spec(spec)
spec.loader.exec_module(t)

S, inv_s = 128, t.SLAB_INV_S
vol, rays = t.small_volume("slab", inv_s), t.slab_rays()
out = oracle.render_fwd(vol, rays, RenderConfig(aabb=t.AABB, n_samples=S, inv_s=inv_s, exact=True), per_sample=True, want_grad_samples=True)
w, sdf, grad = out["weights"].double(), out["sdf"].double(), out["grad"].double()
dt = ((out["fars"] - out["nears"]) / S).double()[:, None]
# certainly a free-space sample: both sigmoid arguments above 17.5 whatever the direction
free = (sdf - grad.norm(dim=-1) * dt * 0.5) * inv_s > 17.6
T = w / float(t.K_ALPHA_FREE)                       # transmittance BEFORE the sample, valid where `free`
idx = torch.arange(S)[None].expand_as(w)
first_sdf_neg = torch.where(sdf < 0, idx, S).min(dim=1).values
behind = free & (idx > first_sdf_neg[:, None])       # free samples after the ray has been inside the slab
reach = behind.any(dim=1)
first_behind = torch.where(behind, idx, S).min(dim=1).values.clamp_max(S - 1)
T_entry = torch.where(reach, T.gather(1, first_behind[:, None])[:, 0], torch.zeros(()).double())
print(f"rays {w.shape[0]}, reaching free space behind the slab: {int(reach.sum())}, "
      f"T there from {float(T_entry[reach].min()):.2e} to {float(T_entry[reach].max()):.2e}")
more = behind & torch.roll(behind, -1, dims=1) & (idx < S - 1)
window = more & (T >= 1e-10) & (T <= 2e-10)
print("rays with T in [1e-10, 2e-10] at a free sample followed by another free sample:", int(window.any(dim=1).sum()))
ny, nx = rays.ny, rays.nx
Te = T_entry.view(ny, nx)
n_hi = n_mid = n_lo = 0
for ty in range(0, ny, 8):
    for tx in range(0, nx, 8):
        m = float(Te[ty:ty + 8, tx:tx + 8].max())
        n_hi += m >= 2e-10
        n_mid += 1e-10 <= m < 2e-10
        n_lo += m < 1e-10
print(f"8 x 8 tiles by their largest T behind the slab: >= 2e-10: {n_hi}, in [1e-10, 2e-10): {n_mid}, < 1e-10: {n_lo}")
if "--map" in sys.argv:
    import math
    for ty in range(0, ny, 4):
        print(" ".join(f"{math.log10(max(float(Te[ty, tx]), 1e-30)):6.1f}" for tx in range(0, nx, 6)))
