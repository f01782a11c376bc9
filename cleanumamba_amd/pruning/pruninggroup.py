"""Prunable channel groups of CleanUMamba: public interface of the reference's src/pruning/pruninggroup.py.

A ``PruningGroup`` is a set of channels that are removed together from several modules (``PruningModule``): the output
rows of one layer and the matching input columns of the layers that read them.  Importances come from one HIP launch
(``device.importances``); pruning goes through ``device.prune_modules``, which keeps a flat-managed model (TrainStep /
FlatAdam) flat.

Row grouping of multi-head modules (``n_heads = 2``: the GLU convs, in_proj, the B / C rows of x_proj), kept as the
reference has it and as the shipped pruned checkpoints were selected: the importance of channel c sums rows
``offset + c * n_heads + h`` (the reference's ``reshape(n_channels, -1)``), while pruning channel c removes rows
``offset + h * n_channels + c``.
"""
import typing

import torch
import torch.nn as nn

_STATISTICS_OUT_OF_SCOPE = ("statistics=True (activation telemetry through forward hooks) is not supported: on the fused "
                            "path the convs and the Mamba projections run inside single autograd nodes, so the hooks "
                            "would never fire")


class ParameterContainer:
    """A bare parameter of a module (``A_log``, ``D``) dressed as a module for PruningModule."""

    def __init__(self, name, module):
        self.name = name
        self.module = module

    @property
    def shape(self):
        return getattr(self.module, self.name).shape

    def __repr__(self):
        return f"{self.name} {self.module}"

    def set(self, value):
        setattr(self.module, self.name, value)

    def get(self):
        return getattr(self.module, self.name)

    def register_forward_hook(self, hook):
        pass

    def register_forward_pre_hook(self, hook):
        pass


PC = ParameterContainer


class PruningModule:
    """One module's share of a group: its ``weight`` (or the contained parameter) along ``dim``, ``n_heads`` row blocks,
    starting ``channel_offset`` rows in.  ``next_module_to_offset``: another PruningModule on the same matrix whose
    offset moves when this one loses rows (x_proj: dt_rank rows before the B / C rows)."""

    def __init__(self, module: typing.Union[nn.Module, ParameterContainer], out=True, dim=0, n_heads=1,
                 channel_offset=0, next_module_to_offset=None, statistics=False):
        supported = (ParameterContainer, nn.Conv1d, nn.ConvTranspose1d, nn.Linear, nn.LayerNorm)
        if not isinstance(module, supported):
            raise TypeError(f"Unsupported module type {module.__class__}")
        if statistics and not isinstance(module, ParameterContainer):
            raise NotImplementedError(_STATISTICS_OUT_OF_SCOPE)
        if next_module_to_offset is not None and next_module_to_offset.module is not module:
            raise ValueError("next_module_to_offset must act on the same matrix")
        self.module = module
        self.dim = dim
        self.n_heads = n_heads
        self.channel_offset = channel_offset
        self.next_module_to_offset = next_module_to_offset
        self.out = out
        self.group = None

    def param(self):
        """The parameter this module prunes."""
        return self.module.get() if isinstance(self.module, ParameterContainer) else self.module.weight

    def bias(self):
        """The bias pruned with the weight (same rows), or None: only along the output dimension, only if it has more than
        one element (reference rule)."""
        if isinstance(self.module, ParameterContainer):
            return None
        b = getattr(self.module, "bias", None)
        out_dim = 1 if isinstance(self.module, nn.ConvTranspose1d) else 0
        if b is None or self.dim != out_dim or b.shape[0] <= 1:
            return None
        return b

    def _next_start(self, rows):
        return 0 if self.next_module_to_offset is None else rows - self.next_module_to_offset.channel_offset

    def check(self, channels):
        rows = self.param().shape[self.dim]
        if rows % self.n_heads != 0:
            raise AssertionError(f"Module channels {rows} % {self.n_heads} != 0")
        if rows / self.n_heads != channels:
            raise AssertionError(f"Module channels {rows} != {channels}")

    def removed_rows(self, idxs, n_channels):
        """Rows along ``dim`` that pruning channels ``idxs`` removes (reference: head h of channel c is row
        offset + h * n_channels + c)."""
        return [self.channel_offset + h * n_channels + c for h in range(self.n_heads) for c in idxs]

    def channel_importances(self):
        """This module's importance dict (one HIP launch for this module alone)."""
        from . import device
        return device.module_importances([self])[0]

    def change_offset(self, change):
        self.channel_offset += change
        if self.next_module_to_offset is not None:
            self.next_module_to_offset.change_offset(change)

    def prune(self, idxs, head=False, optimizer=None):
        """Prune channels ``idxs`` of this module alone (the group's channel count is not changed)."""
        from . import device
        idxs = _as_index_list(idxs)
        if head or self.n_heads == 1:
            rows = [self.channel_offset + i for i in idxs]
        else:
            rows = self.removed_rows(idxs, self.group.n_channels)
        device.prune_modules([(self, rows)], optimizer, model=getattr(self.group, "model", None))
        if self.next_module_to_offset is not None:
            self.next_module_to_offset.change_offset(-len(idxs) * self.n_heads)

    def __repr__(self):
        return f"{self.__class__.__name__} <{str(self)}>"

    def __str__(self):
        return (f"{self.module.__class__.__name__} (dim={self.dim}, n_heads={self.n_heads}, "
                f"channel_offset={self.channel_offset}, telemetry=None)")


def _as_index_list(idxs):
    if isinstance(idxs, torch.Tensor):
        idxs = idxs.reshape(-1).tolist()
    out = []
    for i in idxs:
        if isinstance(i, torch.Tensor):
            i = i.item()
        if isinstance(i, bool) or int(i) != i:
            raise ValueError(f"channel index {i!r} is not an integer")
        out.append(int(i))
    return out


class PruningGroup:
    """Group of pruning modules that are pruned together."""

    min_channels = 1          # a group never loses its last channel

    def __init__(self, name, n_channels, main_module=None, data_len=0):
        self.name = name
        self.n_channels = n_channels
        self.data_len = data_len
        self.main_module = main_module
        self.modules = []
        self.model = None          # the CleanUMamba the group belongs to (its caches are dropped after a prune)

    def add_module(self, module):
        if not isinstance(module, PruningModule):
            raise TypeError("add_module takes a PruningModule")
        self.modules.append(module)
        module.group = self

    def prune(self, idxs, optimizer=None):
        """Remove channels ``idxs``.  ``optimizer``: None, a torch.optim.Adam (its moments are sliced per tensor) or the
        FlatAdam of a TrainStep (the flat buffers are compacted on the device and the parameters stay flat)."""
        from . import device
        device.prune_groups_dict({self: _as_index_list(idxs)}, optimizer)

    def check(self):
        for module in self.modules:
            rows = module.param().shape[module.dim]
            next_start = module._next_start(rows)
            if (rows - module.channel_offset - next_start) // module.n_heads != self.n_channels:
                raise AssertionError(f"{module.module}: ({rows} - {module.channel_offset} - {next_start}) // "
                                     f"{module.n_heads} == {self.n_channels}")

    def channel_importances(self):
        """Importances of this group's channels (one HIP launch for this group; nothing is cached between calls)."""
        from . import device
        return device.group_importances([self])[0]

    def __repr__(self):
        return f"{self.__class__.__name__} <{str(self)}>"

    def __str__(self):
        return f"{self.name} (n_channels={self.n_channels}, modules={[str(m) for m in self.modules]})"


def CleanUMambaPrunableChannels(model, statistics=False):
    """The prunable groups of a CleanUMamba (Mamba1 bottleneck), in the reference's order and with its names:
    encode_down_i, decode_mix_i, skip_conn_i per level, d_model, then d_inner{i}, d_state{i}, dt_rank{i} per block."""
    if statistics:
        raise NotImplementedError(_STATISTICS_OUT_OF_SCOPE)
    for block in model.tsfm_Mamba_layers:
        if not hasattr(block.mixer, "x_proj"):
            raise NotImplementedError("channel pruning covers the Mamba1 bottleneck (mamba_v2=False) only")
    groups = []

    def add(group, modules):
        for m in modules:
            group.add_module(m)
        group.check()
        group.model = model
        groups.append(group)

    PM = PruningModule
    n_enc = len(model.encoder)
    for i in range(n_enc):
        d = len(model.decoder) - i - 1
        add(PruningGroup(f"encode_down_{i}", model.encoder[i][0].weight.shape[0], data_len=80126 // (2 ** i)),
            [PM(model.encoder[i][0], True, dim=0), PM(model.encoder[i][2], False, dim=1)])
        add(PruningGroup(f"decode_mix_{i}", model.decoder[d][0].weight.shape[0] // 2, data_len=80126 // (2 ** i)),
            [PM(model.decoder[d][0], True, n_heads=2, dim=0), PM(model.decoder[d][2], False, dim=0)])
        mods = [PM(model.encoder[i][2], True, n_heads=2, dim=0), PM(model.decoder[d][0], False, dim=1)]
        if i + 1 == n_enc:
            mods += [PM(model.tsfm_conv1, False, dim=1), PM(model.tsfm_conv2, True, dim=0)]
        else:
            mods += [PM(model.encoder[i + 1][0], False, dim=1), PM(model.decoder[d - 1][2], True, dim=1)]
        add(PruningGroup(f"skip_conn_{i}", model.encoder[i][2].weight.shape[0] // 2, data_len=80126 // (2 ** i)), mods)

    mods = [PM(model.tsfm_conv1, True, dim=0), PM(model.tsfm_conv2, False, dim=1), PM(model.norm_f, False, dim=0)]
    for block in model.tsfm_Mamba_layers:
        mods += [PM(block.norm, False, dim=0), PM(block.mixer.in_proj, False, dim=1),
                 PM(block.mixer.out_proj, True, dim=0)]
    add(PruningGroup("d_model", model.tsfm_conv1.weight.shape[0], data_len=624, main_module=model.tsfm_Mamba_layers), mods)

    for i, block in enumerate(model.tsfm_Mamba_layers):
        mx = block.mixer
        add(PruningGroup(f"d_inner{i}", mx.in_proj.weight.shape[0] // 2, data_len=624, main_module=mx),
            [PM(mx.in_proj, True, n_heads=2, dim=0), PM(mx.out_proj, False, dim=1), PM(mx.conv1d, False, dim=0),
             PM(mx.x_proj, False, dim=1), PM(mx.dt_proj, True, dim=0), PM(ParameterContainer("A_log", mx), False, dim=0),
             PM(ParameterContainer("D", mx), True, dim=0)])
        dt_rank = mx.dt_proj.weight.shape[1]
        x_state = PM(mx.x_proj, True, dim=0, n_heads=2, channel_offset=dt_rank)
        add(PruningGroup(f"d_state{i}", mx.A_log.shape[1], data_len=624),
            [x_state, PM(ParameterContainer("A_log", mx), False, dim=1)])
        add(PruningGroup(f"dt_rank{i}", dt_rank, main_module=mx),
            [PM(mx.x_proj, True, dim=0, next_module_to_offset=x_state), PM(mx.dt_proj, True, dim=1)])
    return groups
