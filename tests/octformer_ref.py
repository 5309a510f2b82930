"""Plain torch restatement of the reference's OctFormer statements (pointcept/models/octformer/octformer_v1m1_base.py), for any
dtype: the same function gives the float64 reference and the fp32 eager run.  No logic beyond the statements."""
import torch
import torch.nn.functional as F

INVALID_MASK_VALUE = -1e3


def patch_partition(data, num, fill_value=0):   # :93-96
    tail = data.new_full((num,) + data.shape[1:], fill_value)
    return torch.cat([data, tail], dim=0)


def calc_attn_mask(mask):   # :75-78
    attn_mask = mask.unsqueeze(2) - mask.unsqueeze(1)
    return attn_mask.masked_fill(attn_mask != 0, INVALID_MASK_VALUE)


def attention(qkv, xyz, batch, batch_size, rpe_table, K, D, scale):
    """:56-99, :165-176, :212-245 from the projected qkv (n, 3 C) to the rows patch_reverse keeps.  The padded rows are zeros
    where the reference's hold the qkv bias; they are masked against every real row and cut off at the end."""
    H = rpe_table.shape[1]
    n, C = qkv.shape[0], qkv.shape[1] // 3
    num = -(-n // (K * D)) * (K * D) - n
    pos_bnd = int(0.8 * K * D ** 0.5)
    rpe_num = 2 * pos_bnd + 1
    batch = patch_partition(batch.long(), num, batch_size)
    xyz = patch_partition(xyz.long(), num)
    data = patch_partition(qkv, num)
    if D > 1:
        mask = calc_attn_mask(batch.view(-1, K, D).transpose(1, 2).reshape(-1, K))
        xyz = xyz.view(-1, K, D, 3).transpose(1, 2).reshape(-1, K, 3)
        data = data.view(-1, K, D, 3 * C).transpose(1, 2).reshape(-1, 3 * C)
    else:
        mask = calc_attn_mask(batch.view(-1, K))
        xyz = xyz.view(-1, K, 3)
    rel_pos = xyz.unsqueeze(2) - xyz.unsqueeze(1)

    qkv = data.reshape(-1, K, 3, H, C // H).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * scale
    attn = q @ k.transpose(-2, -1)
    mul = torch.arange(3, device=xyz.device) * rpe_num   # :165-176
    idx = rel_pos.clamp(-pos_bnd, pos_bnd) + (pos_bnd + mul)
    out = rpe_table.index_select(0, idx.reshape(-1))
    out = out.view(idx.shape + (-1,)).sum(3).permute(0, 3, 1, 2)
    attn = attn + out
    attn = attn + mask.unsqueeze(1)
    attn = torch.softmax(attn, dim=-1)
    data = (attn @ v).transpose(1, 2).reshape(-1, C)
    if D > 1:
        data = data.view(-1, D, K, C).transpose(1, 2).reshape(-1, C)
    return data[:n]


def dwconv(x, weights, nbr):
    """y[i, c] = sum_k weights[k, 0, c] x[nbr[i, k], c], -1 skipped"""
    y = torch.zeros_like(x)
    for k in range(27):
        j = nbr[:, k].long()
        y = y + weights[k, 0] * x[j.clamp(min=0)] * (j >= 0).unsqueeze(1).to(x.dtype)
    return y


def block(data, p, xyz, batch, batch_size, nbr, K, D, num_heads):
    """OctFormerBlock.forward :297-303 in training mode, drop_path 0; p: the block's state dict as tensors of one dtype"""
    C = data.shape[1]
    cpe = F.batch_norm(dwconv(data, p["cpe.conv.weights"], nbr), None, None, p["cpe.bn.weight"], p["cpe.bn.bias"], True)
    data = cpe + data
    x = F.layer_norm(data, (C,), p["norm1.weight"], p["norm1.bias"])
    x = attention(F.linear(x, p["attention.qkv.weight"], p["attention.qkv.bias"]), xyz, batch, batch_size,
                  p["attention.rpe.rpe_table"], K, D, (C // num_heads) ** -0.5)
    data = data + F.linear(x, p["attention.proj.weight"], p["attention.proj.bias"])
    x = F.layer_norm(data, (C,), p["norm2.weight"], p["norm2.bias"])
    x = F.linear(F.gelu(F.linear(x, p["mlp.fc1.weight"], p["mlp.fc1.bias"])), p["mlp.fc2.weight"], p["mlp.fc2.bias"])
    return data + x
