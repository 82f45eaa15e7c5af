"""The heuristic network of the reference's mkp_transformer/net.py on MI355X: `TransformerModel`, whose `state_dict()` has the
reference's keys and shapes (45 entries, 21 761 parameters at six input features), so the pretrained checkpoints load
unchanged:

    transformer_encoder.layers.{0,1,2}.{self_attn.in_proj_weight [96,32], self_attn.in_proj_bias, self_attn.out_proj.*,
    linear1.*, linear2.*, norm1.*, norm2.*}, encoder.*, decoder_heu._dummy (empty, frozen), decoder_heu.lins.{0,1,2}.*

With gradients disabled the forward is the HIP encoder (csrc/daco_transformer.hip through engine.transformer_forward; a
missing library is an error, there is no fall-back).  With gradients enabled it is the same encoder's training forward and
mkp_transformer/train.py's loss.backward() runs csrc/daco_transformer_train.hip (autograd.TransformerFn):
`grad_path = "hip"`, the default.  `grad_path = "torch"` runs `_torch_forward`, nn.TransformerEncoder on torch ops built from
the same parameters: the comparator of the tests and of A/B timing.  No gradient reaches `src`.  `forward(src)` takes the
reference's [n, 1, m+1] and returns [n]; `forward_batch` takes [B, n, m+1] and returns [B, n], every sequence divided by its
own maximum.
"""
import math

import torch
from torch import nn
import torch.nn.functional as F

from . import _lib, engine

_LAYER_ORDER = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias",
                "norm2.weight", "norm2.bias")


class MLP(nn.Module):
    @property
    def device(self):
        return self._dummy.device

    def __init__(self, units_list, act_fn):
        super().__init__()
        assert act_fn == 'relu'
        self._dummy = nn.Parameter(torch.empty(0), requires_grad=False)
        self.units_list = units_list
        self.depth = len(units_list) - 1
        self.lins = nn.ModuleList([nn.Linear(units_list[i], units_list[i + 1]) for i in range(self.depth)])

    def forward(self, x):
        for i, lin in enumerate(self.lins):
            x = lin(x)
            x = F.relu(x) if i < self.depth - 1 else torch.sigmoid(x)
        return x


class ParNet(MLP):
    def __init__(self, depth=3, units=32, preds=1, act_fn='relu'):
        self.units, self.preds = units, preds
        super().__init__([units] * depth + [preds], act_fn)

    def forward(self, x):
        return super().forward(x).squeeze(dim=-1)


class TransformerModel(nn.Module):
    grad_path = "hip"          # how a forward with gradients enabled runs: "hip" | "torch" (set on the class or an instance)

    def __init__(self, ntoken_input=6, d_model=32, nhead=2, d_hid=32, nlayers=3, dropout=0):
        super().__init__()
        assert (d_model, nhead, d_hid, nlayers, dropout) == (32, 2, 32, 3, 0), "the HIP encoder is built for the reference's sizes"
        self.model_type = 'Transformer'
        self.transformer_encoder = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model, nhead, d_hid, dropout), nlayers,
                                                         enable_nested_tensor=False)
        self.encoder = nn.Linear(ntoken_input, d_model)
        self.d_model = d_model
        self.decoder_heu = ParNet()
        self.encoder.weight.data.uniform_(-0.1, 0.1)          # mkp_transformer/net.py:29-31

    # ---- the flat parameter block of csrc/daco_transformer.hip
    def _ordered_parameters(self):
        ps = [self.encoder.weight, self.encoder.bias]
        for layer in self.transformer_encoder.layers:
            sd = dict(layer.named_parameters())
            ps += [sd[k] for k in _LAYER_ORDER]
        for lin in self.decoder_heu.lins:
            ps += [lin.weight, lin.bias]
        return ps

    def packed_parameters(self):
        """The flat block, packed from the parameters as they are NOW on every call.  No cache: a write through `.data`
        (net.py:31's own `encoder.weight.data.uniform_`, an EMA's `p.data.copy_`) changes neither `data_ptr()` nor `_version`,
        so nothing cheap tells a stale block from a fresh one; one cat of 44 small tensors is the price."""
        return torch.cat([p.detach().float().reshape(-1) for p in self._ordered_parameters()]).contiguous()

    def packed_parameters_with_grad(self):
        """The same block as a differentiable cat: its backward hands every parameter its slice of the block's gradient."""
        return torch.cat([p.float().reshape(-1) for p in self._ordered_parameters()])

    def _torch_forward(self, src_n_B_f):
        x = self.encoder(src_n_B_f) * math.sqrt(self.d_model)
        heu = self.decoder_heu(self.transformer_encoder(x))            # [n, B]
        return heu / heu.max(dim=0, keepdim=True).values

    def forward_batch(self, src):
        """src [B, n, m+1] -> [B, n]"""
        if not src.is_cuda or not self.encoder.weight.is_cuda:
            raise _lib.DacoError("TransformerModel needs its input and parameters on a HIP device; there is no CPU path")
        if torch.is_grad_enabled():
            if self.grad_path == "torch":
                return self._torch_forward(src.transpose(0, 1)).transpose(0, 1)
            if self.grad_path != "hip":
                raise ValueError(f"grad_path is 'hip' or 'torch', not {self.grad_path!r}")
            from .autograd import TransformerFn
            return TransformerFn.apply(src, self.packed_parameters_with_grad())
        return engine.transformer_forward(src, self.packed_parameters())

    def forward(self, src):
        """src [n, 1, m+1] (mkp_transformer/utils.py reformat) -> [n]"""
        return self.forward_batch(src.transpose(0, 1))[0]
