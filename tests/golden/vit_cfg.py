"""VisionTransformer cases shared by tests/golden/make_golden_g23.py and the tests: (constructor kwargs, batch).  The smallest shapes
at which each code path can still go wrong (1-D / 2-D / 3-D token order, N below one attention tile and N with a ragged last tile,
K = C * p^dims padded to the GEMM width, a hidden width that is no power of two, an odd batch)."""
import torch

from detdata import det_normal

VIT_CASES = {
    "vit1d": (dict(patch_size=4, input_shapes=[64], num_channels=1, embedding_dim=32, hidden_dim=64, activation="SiLU",
                   transformer_depth=1, num_heads=2, dropout=0.0), 2),
    "vit2d": (dict(patch_size=4, input_shapes=[16, 24], num_channels=3, embedding_dim=64, hidden_dim=96, activation="GELU",
                   transformer_depth=2, num_heads=2, dropout=0.0), 3),
    "vit3d": (dict(patch_size=2, input_shapes=[8, 4, 12], num_channels=2, embedding_dim=64, hidden_dim=128, activation="GELU",
                   transformer_depth=2, num_heads=4, dropout=0.0), 2),
    "vit2d_long": (dict(patch_size=2, input_shapes=[32, 40], num_channels=1, embedding_dim=32, hidden_dim=32, activation="ReLU",
                        transformer_depth=1, num_heads=1, dropout=0.0), 2),
}


def vit_inputs(case: str):
    """(kwargs, x, t, target) of a case: det_normal inputs, timesteps [3, 17, 41][:B]."""
    kw, B = VIT_CASES[case]
    shape = (B, kw["num_channels"], *kw["input_shapes"])
    return dict(kw), det_normal(shape, case + "x"), torch.tensor([3, 17, 41][:B]), det_normal(shape, case + "tgt")
