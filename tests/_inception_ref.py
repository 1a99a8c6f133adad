"""An independent CPU oracle for the FID InceptionV3 (pool3 features): the network restated with torch.nn.functional calls
in NCHW, written out block by block from the published architecture (torchvision's Inception3 with pytorch-fid's FID
variants of the A / C / E blocks).  It takes a state dict in torchvision's names and a dtype, and imports nothing from
commonscenes_amd."""
import torch
import torch.nn.functional as F

EPS = 1e-3


def basic_conv(sd, name, x, stride=1, padding=0):
    """BasicConv2d: conv without bias, eval-mode BatchNorm(eps 1e-3), ReLU"""
    dt = x.dtype
    g = lambda k: sd[f"{name}.{k}"].to(dt)
    y = F.conv2d(x, g("conv.weight"), None, stride=stride, padding=padding)
    y = F.batch_norm(y, g("bn.running_mean"), g("bn.running_var"), g("bn.weight"), g("bn.bias"), training=False, eps=EPS)
    return F.relu(y)


def avg3(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


def block_a(sd, n, x):
    b1 = basic_conv(sd, f"{n}.branch1x1", x)
    b5 = basic_conv(sd, f"{n}.branch5x5_2", basic_conv(sd, f"{n}.branch5x5_1", x), padding=2)
    b3 = basic_conv(sd, f"{n}.branch3x3dbl_1", x)
    b3 = basic_conv(sd, f"{n}.branch3x3dbl_2", b3, padding=1)
    b3 = basic_conv(sd, f"{n}.branch3x3dbl_3", b3, padding=1)
    bp = basic_conv(sd, f"{n}.branch_pool", avg3(x))
    return [b1, b5, b3, bp]


def block_b(sd, n, x):
    b3 = basic_conv(sd, f"{n}.branch3x3", x, stride=2)
    bd = basic_conv(sd, f"{n}.branch3x3dbl_1", x)
    bd = basic_conv(sd, f"{n}.branch3x3dbl_2", bd, padding=1)
    bd = basic_conv(sd, f"{n}.branch3x3dbl_3", bd, stride=2)
    return [b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)]


def block_c(sd, n, x):
    b1 = basic_conv(sd, f"{n}.branch1x1", x)
    b7 = basic_conv(sd, f"{n}.branch7x7_1", x)
    b7 = basic_conv(sd, f"{n}.branch7x7_2", b7, padding=(0, 3))
    b7 = basic_conv(sd, f"{n}.branch7x7_3", b7, padding=(3, 0))
    bd = basic_conv(sd, f"{n}.branch7x7dbl_1", x)
    bd = basic_conv(sd, f"{n}.branch7x7dbl_2", bd, padding=(3, 0))
    bd = basic_conv(sd, f"{n}.branch7x7dbl_3", bd, padding=(0, 3))
    bd = basic_conv(sd, f"{n}.branch7x7dbl_4", bd, padding=(3, 0))
    bd = basic_conv(sd, f"{n}.branch7x7dbl_5", bd, padding=(0, 3))
    bp = basic_conv(sd, f"{n}.branch_pool", avg3(x))
    return [b1, b7, bd, bp]


def block_d(sd, n, x):
    b3 = basic_conv(sd, f"{n}.branch3x3_2", basic_conv(sd, f"{n}.branch3x3_1", x), stride=2)
    b7 = basic_conv(sd, f"{n}.branch7x7x3_1", x)
    b7 = basic_conv(sd, f"{n}.branch7x7x3_2", b7, padding=(0, 3))
    b7 = basic_conv(sd, f"{n}.branch7x7x3_3", b7, padding=(3, 0))
    b7 = basic_conv(sd, f"{n}.branch7x7x3_4", b7, stride=2)
    return [b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)]


def block_e(sd, n, x, pool):
    b1 = basic_conv(sd, f"{n}.branch1x1", x)
    b3 = basic_conv(sd, f"{n}.branch3x3_1", x)
    b3 = torch.cat([basic_conv(sd, f"{n}.branch3x3_2a", b3, padding=(0, 1)),
                    basic_conv(sd, f"{n}.branch3x3_2b", b3, padding=(1, 0))], 1)
    bd = basic_conv(sd, f"{n}.branch3x3dbl_1", x)
    bd = basic_conv(sd, f"{n}.branch3x3dbl_2", bd, padding=1)
    bd = torch.cat([basic_conv(sd, f"{n}.branch3x3dbl_3a", bd, padding=(0, 1)),
                    basic_conv(sd, f"{n}.branch3x3dbl_3b", bd, padding=(1, 0))], 1)
    pooled = avg3(x) if pool == "avg" else F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
    bp = basic_conv(sd, f"{n}.branch_pool", pooled)
    return [b1, b3, bd, bp]


BLOCK_FNS = {"A": block_a, "B": block_b, "C": block_c, "D": block_d,
             "E_avg": lambda sd, n, x: block_e(sd, n, x, "avg"), "E_max": lambda sd, n, x: block_e(sd, n, x, "max")}
NETWORK = [("Mixed_5b", "A"), ("Mixed_5c", "A"), ("Mixed_5d", "A"), ("Mixed_6a", "B"), ("Mixed_6b", "C"), ("Mixed_6c", "C"),
           ("Mixed_6d", "C"), ("Mixed_6e", "C"), ("Mixed_7a", "D"), ("Mixed_7b", "E_avg"), ("Mixed_7c", "E_max")]


def block(sd, name, kind, x_nchw):
    """the list of branch outputs (NCHW) of one Mixed block"""
    return BLOCK_FNS[kind](sd, name, x_nchw)


@torch.no_grad()
def features(sd, x_nhwc, dtype=torch.float64):
    """x_nhwc: [B, H, W, >= 3] normalised input (channels past 2 are ignored) -> pool3 features [B, 2048] in `dtype`"""
    x = x_nhwc[..., :3].to(dtype).permute(0, 3, 1, 2).contiguous()
    x = basic_conv(sd, "Conv2d_1a_3x3", x, stride=2)
    x = basic_conv(sd, "Conv2d_2a_3x3", x)
    x = basic_conv(sd, "Conv2d_2b_3x3", x, padding=1)
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    x = basic_conv(sd, "Conv2d_3b_1x1", x)
    x = basic_conv(sd, "Conv2d_4a_3x3", x)
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    for name, kind in NETWORK:
        x = torch.cat(block(sd, name, kind, x), 1)
    return F.adaptive_avg_pool2d(x, (1, 1)).flatten(1)


def front_end(images_u8, norm, resize=True, dtype=torch.float64):
    """uint8 [B, H, W, 3] -> [B, 299, 299, 3] in `dtype`: F.interpolate(bilinear, align_corners=False) on the 0..255
    values, then 2 (v / 255) - 1 (norm 0) or (v - 128) / 128 (norm 1)"""
    x = images_u8.to(dtype).permute(0, 3, 1, 2)
    if resize:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    x = 2 * (x / 255) - 1 if norm == 0 else (x - 128) / 128
    return x.permute(0, 2, 3, 1).contiguous()
