"""AdamW over the flat parameter buffer of FlatDataParallel.

Same update as torch.optim.AdamW with the reference's two parameter groups
(tools/builder.py:41-101: no weight decay for 1-D tensors, '.bias' and 'token'),
run as two launches of the fused kernel (csrc/adamw.hip) instead of ~35
multi-tensor launches over 203 tensors.  Exposes `param_groups` (so the
reference's schedulers drive `lr` unchanged), `step`, `zero_grad`,
`state_dict` / `load_state_dict` in torch.optim.AdamW's layout: per-parameter `step` /
`exp_avg` / `exp_avg_sq` entries numbered the way the reference's groups number them
(module.named_parameters() order inside each group), so a checkpoint moves between this
optimiser and torch.optim.AdamW over tools/builder.py's groups, and does not depend on how
FlatDataParallel lays the flat buffer out.

`part` selects the reference's other protocols (tools/builder.py:41-98, builder.add_weight_decay): 'only_new' -- two
groups over the parameters whose name contains 'cls', everything else frozen -- and 'diff_lr' -- four groups, the
pretrained parameters at 0.1 x lr (and, as the reference builds them, two empty ones).  The flat layout stays the one of
part 'all'; each group is the list of contiguous
runs its parameters form in it, and ONE launch of pdae_adamw_step_segments updates all of them (8 segments per
launch).  Parameters outside the groups are never touched and have no state entry.
"""
import torch

from . import _lib


_TORCH_GROUP_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False,
                             fused=None, decoupled_weight_decay=True)


def _runs(spans):
    """Sorted (offset, count) spans -> the contiguous runs they form."""
    out = []
    for off, cnt in spans:
        if cnt == 0:
            continue
        if out and out[-1][0] + out[-1][1] == off:
            out[-1] = (out[-1][0], out[-1][1] + cnt)
        else:
            out.append((off, cnt))
    return out


class FlatAdamW:
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, part='all'):
        self.model = model
        self.part = part
        flat = model.flat_param
        if not flat.is_cuda:
            raise RuntimeError('FlatAdamW needs the parameters on the GPU (no CPU path)')
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.steps = 0
        where = dict(zip(model.names, model.offsets))
        if part == 'all':
            nd0, nd1 = model.no_decay_range
            d0, d1 = model.decay_range
            groups = model.param_groups(weight_decay)
            self.param_groups = [
                dict(groups[0], lr=lr, betas=betas, eps=eps, range=(nd0, nd1)),
                dict(groups[1], lr=lr, betas=betas, eps=eps, range=(d0, d1)),
            ]
            named = [n for n, p in model.module.named_parameters() if p.requires_grad]
            k = len(groups[0]['params'])
            nd_names = set(model.names[:k])
            # the parameter names of each group in the reference's order (named_parameters() order inside a group)
            self.group_names = [[n for n in named if n in nd_names], [n for n in named if n not in nd_names]]
        else:
            from .builder import add_weight_decay
            name_of = {id(p): n for n, p in model.module.named_parameters()}
            self.param_groups, self.group_names = [], []
            for g in add_weight_decay(model.module, weight_decay, part=part, lr=lr):
                names = [name_of[id(p)] for p in g['params']]
                self.group_names.append(names)
                self.param_groups.append(dict(g, lr=g.get('lr', lr), betas=betas, eps=eps,
                                              segments=_runs(sorted(where[n] for n in names))))
        for g in self.param_groups:
            g.setdefault('initial_lr', g['lr'])

    def _step_segments(self, grad_scale):
        m = self.model
        table = [(off, cnt, g['lr'], g['weight_decay']) for g in self.param_groups for off, cnt in g['segments']]
        g0 = self.param_groups[0]
        for g in self.param_groups:
            if (g['betas'], g['eps']) != (g0['betas'], g0['eps']):
                raise NotImplementedError('FlatAdamW: one betas / eps for every group (the launch takes one)')
        _lib.adamw_step_segments(m.flat_param, m.flat_grad, self.exp_avg, self.exp_avg_sq, table, g0['betas'][0],
                                 g0['betas'][1], g0['eps'], self.steps, grad_scale)

    def step(self, grad_scale=None):
        """grad_scale: an optional fp32 device scalar the gradients are multiplied by before the update (the
        coefficient of finetune_ops.GradNormClip, i.e. clip_grad_norm_ then step) -- read on the device."""
        self.steps += 1
        m = self.model
        if grad_scale is not None:
            _lib.require(grad_scale, 'grad_scale')
            if grad_scale.numel() != 1:
                raise ValueError('FlatAdamW.step: grad_scale must be a one-element tensor')
        if self.part != 'all':
            return self._step_segments(grad_scale)
        for g in self.param_groups:
            a, b = g['range']
            if b <= a:
                continue
            args = (m.flat_param, b - a, m.flat_param[a:].data_ptr(),
                    m.flat_grad[a:].data_ptr(), self.exp_avg[a:].data_ptr(), self.exp_avg_sq[a:].data_ptr(),
                    float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']),
                    float(g['weight_decay']), self.steps)
            if grad_scale is None:
                _lib.call('pdae_adamw_step', *args)
            else:
                _lib.call('pdae_adamw_step_gscale', *args, grad_scale.data_ptr())

    def zero_grad(self, set_to_none=False):
        self.model.zero_grad()

    def _torch_order(self):
        """[(torch id, flat offset, numel, shape)] -- ids follow the reference's groups (for part 'all': no-decay
        parameters first, then the decayed ones), each in named_parameters() order -- and the first id of each group
        (one entry more than there are groups)."""
        m = self.model
        where = {n: (off, cnt, p.shape) for n, (off, cnt), p in zip(m.names, m.offsets, m.params)}
        order = [n for names in self.group_names for n in names]
        starts = [0]
        for names in self.group_names:
            starts.append(starts[-1] + len(names))
        return [(i,) + where[n] for i, n in enumerate(order)], starts

    def state_dict(self):
        order, starts = self._torch_order()
        state = {}
        if self.steps > 0:
            for i, off, cnt, shape in order:
                state[i] = {'step': torch.tensor(float(self.steps)),
                            'exp_avg': self.exp_avg[off:off + cnt].reshape(shape).clone(),
                            'exp_avg_sq': self.exp_avg_sq[off:off + cnt].reshape(shape).clone()}
        groups = []
        for gi, g in enumerate(self.param_groups):
            d = {key: v for key, v in g.items() if key not in ('params', 'range', 'segments')}
            for key, v in _TORCH_GROUP_DEFAULTS.items():      # so torch.optim.AdamW can load the groups
                d.setdefault(key, v)
            d['params'] = list(range(starts[gi], starts[gi + 1]))
            groups.append(d)
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd):
        order, _ = self._torch_order()
        state = sd['state']
        if state and 'exp_avg' in state and not isinstance(state['exp_avg'], dict):
            raise RuntimeError('FlatAdamW.load_state_dict: flat-layout optimiser state of an earlier build; '
                               'checkpoints now use torch.optim.AdamW\'s per-parameter layout')
        self.exp_avg.zero_(), self.exp_avg_sq.zero_()
        steps = set()
        for i, off, cnt, shape in order:
            st = state.get(i, state.get(str(i)))
            if st is None:
                continue
            self.exp_avg[off:off + cnt].copy_(st['exp_avg'].reshape(-1))
            self.exp_avg_sq[off:off + cnt].copy_(st['exp_avg_sq'].reshape(-1))
            steps.add(int(st['step']))
        if len(steps) > 1:
            raise RuntimeError('FlatAdamW.load_state_dict: parameters with different step counts %s '
                               '(the fused update keeps one counter)' % sorted(steps))
        self.steps = steps.pop() if steps else 0
        for g, saved in zip(self.param_groups, sd['param_groups']):
            g.update({key: v for key, v in saved.items()
                      if key not in ('params', 'range', 'segments') and key not in _TORCH_GROUP_DEFAULTS})
