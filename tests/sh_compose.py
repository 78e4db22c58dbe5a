"""float64 composition of a spherical-harmonics render from parts that the feature does not touch: the differentiable torch
port of the march (weights / acc / sample positions, SDF channel only), its explicit trilinear lookup on the coefficient
volume at the same positions, the fixture-pinned basis (selfocc_amd.sh, tests/test_sh_cpu.py), the activation, the
background and the clamp.  Differentiable with respect to sdf64 / feat64 / inv_s64."""
import torch

from oracle import torch_port as tp
from selfocc_amd import sh


def compose64(mapping, sdf64, feat64, sh_deg, sh_act, ex, cfg, inv_s64, t_rand=None, bkgd_rays=None,
              slope_eps=None, slope_f64=False, drop_corner=None):
    """sdf64 (H, W, D), feat64 (H, W, D, F) float64; ex: explicit RaySet on the CPU.  Returns the port's dict + 'rgb' and the
    raw colour 'raw' (n_rays, S, 3) before the activation.  Works in the dtype of ``sdf64`` (float32 volumes give the float32
    yardstick of tests/render_bwd_cases.py).  ``slope_eps`` / ``slope_f64`` / ``drop_corner``: see tp.trilinear_explicit."""
    dd = sdf64.dtype
    o, d, dn = ex.origins.to(dd), ex.dirs.to(dd), ex.dir_norm.to(dd)
    out = tp.render_port_differentiable(mapping, sdf64[None], 0, 0, o, d, dn, cfg, inv_s64,
                                        None if t_rand is None else t_rand.to(dd), None, slope_eps, slope_f64, drop_corner)
    S = cfg.n_samples
    at = out['starts'] if cfg.sample_pos == 0 else (out['starts'] + out['ends']) / 2
    pos = o[:, None, :] + d[:, None, :] * at[..., None]
    f, _ = tp.trilinear_explicit(mapping, feat64.permute(3, 0, 1, 2), pos.reshape(-1, 3), slope_eps, slope_f64, drop_corner)
    nb = sh.n_basis(sh_deg)
    raw = (f[:, :3 * nb].reshape(-1, S, 3, nb) * sh.sh_basis(sh_deg, d)[:, None, None, :]).sum(-1)
    col = torch.relu(raw + 0.5) if sh_act == 'relu' else torch.sigmoid(raw)
    rgb = (out['weights'][..., None] * col).sum(-2)
    if cfg.bkgd_mode == 1:
        rgb = rgb + torch.tensor(cfg.bkgd, dtype=dd) * (1.0 - out['acc'][:, None])
    elif cfg.bkgd_mode == 2:
        rgb = rgb + bkgd_rays.to(dd) * (1.0 - out['acc'][:, None])
    if cfg.clamp_rgb:
        rgb = rgb.clamp(0.0, 1.0)
    out['rgb'] = rgb
    out['raw'] = raw
    return out
