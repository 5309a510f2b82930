"""Host: SPVCNN's state dict carries the reference's (torchsparse's) keys and shapes."""


def test_state_dict_keys_and_shapes():
    from ao_amd.spvcnn import SPVCNN

    sd = SPVCNN(6, 13).state_dict()
    shapes = {"stem.0.kernel": (27, 6, 32), "stage1.0.net.0.kernel": (8, 32, 32), "up1.1.0.downsample.0.kernel": (384, 256),
              "point_transforms.0.0.weight": (256, 32), "classifier.0.weight": (13, 96), "classifier.0.bias": (13,),
              "stage2.1.downsample.0.kernel": (32, 64), "up4.0.net.0.kernel": (8, 96, 96), "stem.1.running_var": (32,)}
    assert {k: tuple(sd[k].shape) for k in shapes} == shapes
    assert not [k for k in sd if k.startswith("stage1.1.downsample")]   # inc == outc: nn.Identity
    tops = {k.split(".")[0] for k in sd}
    assert tops == {"stem", "classifier", "point_transforms"} | {"stage%d" % i for i in range(1, 5)} | {"up%d" % i for i in range(1, 5)}
    bn = {"weight", "bias", "running_mean", "running_var", "num_batches_tracked"}
    assert {k.rsplit(".", 1)[1] for k in sd if k.startswith("stem.1.")} == bn
    # every leaf is a kernel (convolutions, no bias), a BatchNorm1d key or a Linear's weight / bias
    assert {k.rsplit(".", 1)[1] for k in sd} == bn | {"kernel"}

