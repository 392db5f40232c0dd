"""Float64 references of the dense, loss and small-op kernels (csrc/tabular.hip, cf_ops.hip, the end of pointwise.hip): what
tests/test_hip_small_ops.py compares the HIP kernels with.  Plain torch on the CPU, every backward written out by hand;
tests/test_small_ops_plan_host.py pins the hand-written ones to torch.float64 autograd, so a wrong reference fails there and not on
the GPU.  Each function takes float64 tensors (the test rounds its inputs to float32 first, so these see the kernel's operands) and,
where a test needs an error bound, also returns the magnitude sum sum|terms| the bound scales with."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24        # unit roundoff of float32


def f32_exact(t):
    """float64 values that are exactly representable in float32."""
    return t.float().double()


# ---- GEMM ----------------------------------------------------------------------------------------------------------------------
def gemm(A, B, transA, transB, bias=None, C0=None, leaky=None):
    """(act(opA opB + bias + C0), |opA| |opB| + |bias| + |C0|)"""
    a = A.T if transA else A
    b = B.T if transB else B
    out, mag = a @ b, a.abs() @ b.abs()
    if bias is not None:
        out, mag = out + bias, mag + bias.abs()
    if C0 is not None:
        out, mag = out + C0, mag + C0.abs()
    if leaky is not None:
        out = torch.where(out > 0, out, out * leaky)
    return out, mag


def linear_wgrad(dy, x, dW0=None, db0=None):
    """(dW, db, sum|terms| of dW, sum|terms| of db): dW = dy^T x (+ dW0), db = column sums of dy (+ db0)"""
    dW, mW = dy.T @ x, dy.abs().T @ x.abs()
    db, mb = dy.sum(0), dy.abs().sum(0)
    if dW0 is not None:
        dW, mW = dW + dW0, mW + dW0.abs()
    if db0 is not None:
        db, mb = db + db0, mb + db0.abs()
    return dW, db, mW, mb


# ---- losses and metrics ----------------------------------------------------------------------------------------------------------
def cross_entropy(z, t, weight=None, grad_scale=1.0, grad_out=1.0):
    """nn.CrossEntropyLoss(weight), reduction mean: (loss, grad_scale * grad_out * d loss / d z)"""
    B, K = z.shape
    lse = torch.logsumexp(z, 1)
    rows = lse - z[torch.arange(B), t]
    w = weight[t] if weight is not None else torch.ones(B, dtype=z.dtype)
    wsum = w.sum()
    loss = (w * rows).sum() / wsum
    onehot = F.one_hot(t, K).to(z.dtype)
    dz = (grad_scale * grad_out / wsum) * w[:, None] * (torch.exp(z - lse[:, None]) - onehot)
    return loss, dz


def cf_metric_rows(lcf, t, lref=None, other=None):
    """Per row: (argmax of logits_cf == target, softmax(lcf)[target] - q); q = softmax(lref)[target] or softmax(lcf)[other].
    Works in the dtype of its inputs (float64: the truth; float32: what fp32 arithmetic on the CPU gives)."""
    B = lcf.shape[0]
    rows = torch.arange(B)
    p = torch.softmax(lcf, 1)
    q = torch.softmax(lref, 1)[rows, t] if lref is not None else p[rows, other]
    return torch.argmax(lcf, 1) == t, p[rows, t] - q


# ---- reductions ------------------------------------------------------------------------------------------------------------------
def am_weight(a, m=None, one_minus=False):
    return torch.ones_like(a) if m is None else (1.0 - m if one_minus else m)


def abs_mean(a, m=None, one_minus=False):
    """(mean |a w|, sum |a w|)"""
    v = (a * am_weight(a, m, one_minus)).abs()
    return v.mean(), v.sum()


def abs_mean_bwd(a, m, one_minus, grad_out, scale=1.0, da0=None):
    w = am_weight(a, m, one_minus)
    da = (grad_out * scale / a.numel()) * torch.sign(a * w) * w
    return da if da0 is None else da0 + da


def norm_sum(flat, seg):
    """sum over the (offset, length) rows of seg of ||flat[offset : offset + length]||_2"""
    return sum((flat[o:o + n].square().sum().sqrt() for o, n in seg), torch.zeros((), dtype=flat.dtype))


# ---- embedding ----------------------------------------------------------------------------------------------------------------------
def embed_concat_fwd(x, idx, table, mask=None):
    ch = [x, table[idx]] + ([mask] if mask is not None else [])
    return torch.stack(ch, dim=-1)


def embed_table_grad(dinp, idx, K, ch=1, base=None):
    """(dtable, sum|terms|): dtable[k] = (base[k] +) sum over the rows b with idx[b] == k of dinp[b, :, ch]"""
    HW = dinp.shape[1]
    d = dinp[..., ch]
    dt = torch.zeros(K, HW, dtype=dinp.dtype).index_add_(0, idx, d)
    mag = torch.zeros(K, HW, dtype=dinp.dtype).index_add_(0, idx, d.abs())
    if base is not None:
        dt, mag = dt + base, mag + base.abs()
    return dt, mag


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
def avgpool_fwd(x):
    """[B, HW, C] -> [B, C]"""
    return x.mean(1)


def avgpool_bwd(dy, HW):
    """[B, C] -> [B, HW, C]"""
    return (dy / HW)[:, None, :].expand(-1, HW, -1).contiguous()
