"""field_volume_train_supported: which field configurations take the fused forward + backward pair under autograd."""
import torch

from selfocc_amd.field import field_volume_supported, field_volume_train_supported


def test_train_support_follows_the_inference_widths():
    for C in (64, 96, 128):
        assert field_volume_train_supported(C, 2, 25, 24, torch.float32)
        assert field_volume_train_supported(C, 2, 1, 0, torch.float32, (257, 257, 31))
        assert field_volume_train_supported(C, 2, 32, 31, torch.float32)
        assert field_volume_supported(C, 2, 25, 24)


def test_train_support_refusals():
    assert not field_volume_train_supported(80, 2, 25, 24, torch.float32)
    assert not field_volume_train_supported(256, 2, 25, 24, torch.float32)
    for C in (64, 96, 128):
        assert not field_volume_train_supported(C, 1, 25, 24, torch.float32)       # density_layers = 1
        assert not field_volume_train_supported(C, 3, 25, 24, torch.float32)       # density_layers = 3
        assert not field_volume_train_supported(C, 2, 33, 31, torch.float32)       # out_dim = 33
        assert not field_volume_train_supported(C, 2, 0, 0, torch.float32)
        assert not field_volume_train_supported(C, 2, 25, 24, torch.bfloat16)      # a bfloat16 feature volume
        assert not field_volume_train_supported(C, 2, 25, 32, torch.float32)       # feature rows wider than 31
