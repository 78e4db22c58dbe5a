"""Learned query lifters (config surface only — no image math):
TPVQueryLifter <- model/lifter/tpv_query_lifter.py:7-36, BEVQueryLifter <- bev_query_lifter.py:7-26,
TPVPositionLifter <- tpv_pos_lifter.py:6-86 (queries = three Linears of constant Fourier features of the plane metres)."""
import torch
import torch.nn as nn

from ..registry import MODELS
from .bricks import BaseModule, TallLinear


@MODELS.register_module()
class TPVQueryLifter(BaseModule):
    def __init__(self, tpv_h, tpv_w, tpv_z, dim, init_cfg=None, **kwargs):
        super().__init__(init_cfg)
        self.tpv_h, self.tpv_w, self.tpv_z, self.dim = tpv_h, tpv_w, tpv_z, dim
        self.tpv_hw = nn.Parameter(torch.randn(1, tpv_h * tpv_w, dim))
        self.tpv_zh = nn.Parameter(torch.randn(1, tpv_z * tpv_h, dim))
        self.tpv_wz = nn.Parameter(torch.randn(1, tpv_w * tpv_z, dim))

    def forward(self, ms_img_feats, *args, **kwargs):
        bs = ms_img_feats[0].shape[0]
        params = (self.tpv_hw, self.tpv_zh, self.tpv_wz)
        if bs == 1 and not torch.is_grad_enabled() and params[0].is_cuda:
            # inference: the planes as views of ONE concatenated tensor (kept until a parameter changes), the form the
            # encoder's first step wants (tpvformer._Planes): no per-frame batch copies, no concatenating copy
            from .encoder.tpvformer import _as_planes
            key = tuple((None if p.is_inference() else p._version, p.data_ptr()) for p in params)
            hit = getattr(self, '_cat_cache', None)
            if hit is None or hit[0] != key:
                hit = self._cat_cache = (key, torch.cat([p.detach() for p in params], 1))
            return {'representation': _as_planes(hit[1], [p.shape[1] for p in params])}
        # read-only downstream: an expanded view instead of the reference's .repeat (a copy, and a reduction in its backward)
        return {'representation': [p.expand(bs, -1, -1) for p in params]}


@MODELS.register_module()
class BEVQueryLifter(BaseModule):
    def __init__(self, bev_h, bev_w, dim, init_cfg=None, **kwargs):
        super().__init__(init_cfg)
        self.bev_h, self.bev_w, self.dim = bev_h, bev_w, dim
        self.bev = nn.Parameter(torch.randn(1, bev_h * bev_w, dim))

    def forward(self, ms_img_feats, *args, **kwargs):
        bs = ms_img_feats[0].shape[0]
        return {'representation': self.bev.to(ms_img_feats[0].dtype).expand(bs, -1, -1)}


@MODELS.register_module()
class TPVPositionLifter(BaseModule):
    """TPV queries from Fourier features of the plane cells' metres (normalised by ``tot_range``; pi * 2^k, k = -1 .. F-2,
    [coord][freq][sin, cos]) through one Linear per plane.  The features are constants of the mapping (non-persistent
    buffers, as in the reference); the Linears are ``TallLinear`` (nn.Linear's keys; the row-split weight gradient the
    encoder's TPVPositionalEncoding uses for the same tall, narrow shapes)."""

    def __init__(self, embed_dims, tot_range, num_freqs, mapping_args, init_cfg=None, **kwargs):
        super().__init__(init_cfg)
        from ..mapping import GridMeterMapping
        from .encoder.tpvformer import _fourier, _normalise, tpv_plane_grids, tpv_plane_meters
        assert isinstance(tot_range, list) and len(tot_range) == 6
        self.mapping = GridMeterMapping(**mapping_args)
        r = tot_range
        hw, zh, wz = tpv_plane_meters(self.mapping, tpv_plane_grids(self.mapping.size_h, self.mapping.size_w, self.mapping.size_d))
        self.register_buffer('hw_freq_feat', _fourier(num_freqs[0], _normalise(hw, r[0], r[3], r[1], r[4])), False)
        self.register_buffer('zh_freq_feat', _fourier(num_freqs[1], _normalise(zh, r[1], r[4], r[2], r[5])), False)
        self.register_buffer('wz_freq_feat', _fourier(num_freqs[2], _normalise(wz, r[0], r[3], r[2], r[5])), False)
        self.position_layer_hw = TallLinear(4 * num_freqs[0], embed_dims)
        self.position_layer_zh = TallLinear(4 * num_freqs[1], embed_dims)
        self.position_layer_wz = TallLinear(4 * num_freqs[2], embed_dims)

    def _planes(self):
        return [self.position_layer_hw(self.hw_freq_feat), self.position_layer_zh(self.zh_freq_feat),
                self.position_layer_wz(self.wz_freq_feat)]

    def forward(self, ms_img_feats, *args, **kwargs):
        bs = ms_img_feats[0].shape[0]
        params = [p for l in (self.position_layer_hw, self.position_layer_zh, self.position_layer_wz) for p in (l.weight, l.bias)]
        if bs == 1 and not torch.is_grad_enabled() and params[0].is_cuda:
            # inference: the queries are a function of the parameters alone, so the Linears run once per parameter state and
            # the planes are views of ONE concatenated tensor (TPVQueryLifter above: tpvformer._Planes takes .cat uncopied)
            from .encoder.tpvformer import _as_planes
            key = tuple((None if p.is_inference() else p._version, p.data_ptr()) for p in params)
            hit = getattr(self, '_cat_cache', None)
            if hit is None or hit[0] != key:
                planes = self._planes()
                hit = self._cat_cache = (key, torch.cat(planes, 0)[None], [p.shape[0] for p in planes])
            return {'representation': _as_planes(hit[1], hit[2])}
        # read-only downstream: an expanded view instead of the reference's .repeat
        return {'representation': [p.unsqueeze(0).expand(bs, -1, -1) for p in self._planes()]}
