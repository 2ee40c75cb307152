"""The task-affinity protocol's linear probe on the gfx950 kernels of csrc/affinity.hip.

The reference (tools/runner_finetune.py:1198-1269) trains nn.Linear(feat_dim, num_class) on the frozen encoder's train
features -- 300 epochs of floor(n / 64) batches of 64, a fresh torch.randperm per epoch, AdamW(lr=1e-3,
weight_decay=0.05), CosineAnnealingLR(T_max=300) stepped once per epoch -- and reports the accuracy and the mean
cross-entropy on the test features; its paper ranks corruptions by that loss.  Here

    W, b = train_linear_probe(train_feats, train_labels, num_class)       # pdae_linear_probe_train: one launch per step
    acc, loss = evaluate(W, b, test_feats, test_labels)                   # pdae_linear_probe_eval

PDAE_AFFINITY=hip (default) selects these kernels, PDAE_AFFINITY=torch the reference's own loop as framework ops on the
device; task_affinity_loss() dispatches.  Both backends share the host-side draws, so that at one seed they see the same
initial values and the same batches and the default host generator is consumed in the reference's order: the init is
torch.nn.Linear(D, K) constructed on the CPU (the reference's Net() before .cuda()), then one torch.randperm(n) per epoch
in epoch order (training draws nothing else from the host generator).  The learning rate of epoch e is
lr (1 + cos(pi e / t_max)) / 2 in fp64 (cosine_lrs).
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib

BATCH = _lib.CONST['PDAE_PROBE_BATCH']
BETAS, EPS = (0.9, 0.999), 1e-8                       # torch.optim.AdamW's defaults, which the reference keeps


def backend():
    """'hip' or 'torch', from PDAE_AFFINITY."""
    name = os.environ.get('PDAE_AFFINITY', 'hip')
    if name not in ('hip', 'torch'):
        raise ValueError('PDAE_AFFINITY=%r: hip or torch' % name)
    return name


def cosine_lrs(lr, t_max, epochs):
    """The learning rate of every epoch under CosineAnnealingLR(T_max=t_max, eta_min=0) stepped once per epoch, fp64:
    lr (1 + cos(pi e / t_max)) / 2, evaluated as the scheduler evaluates it -- each epoch's value from the one before,
    lr_e = lr_{e-1} (1 + cos(pi e / T)) / (1 + cos(pi (e - 1) / T)) -- so that the values are the reference's own.  (The
    closed form evaluated directly is within 4.4e-19 of it over 300 epochs, 1.7e-15 relative.)"""
    out = []
    for e in range(epochs):
        if e == 0:
            cur = float(lr)
        elif (e - 1 - t_max) % (2 * t_max) == 0:        # the restart behind a zero of the cosine
            cur = cur + lr * (1 - math.cos(math.pi / t_max)) / 2
        else:
            cur = (1 + math.cos(math.pi * e / t_max)) / (1 + math.cos(math.pi * (e - 1) / t_max)) * cur
        out.append(cur)
    return out


def draw_init(D, K):
    """The reference's Net(): nn.Linear(D, K) on the CPU under the current torch seed -> (weight (K, D), bias (K,))."""
    lin = torch.nn.Linear(D, K)
    return lin.weight.detach().clone(), lin.bias.detach().clone()


def draw_perms(n, epochs):
    """One torch.randperm(n) per epoch on the default CPU generator, in epoch order -> (epochs, n) int64."""
    if epochs == 0:
        return torch.empty((0, n), dtype=torch.int64)
    return torch.stack([torch.randperm(n) for _ in range(epochs)], 0)


def _host_labels(labels, count, num_class, name):
    """labels -> (count,) int64 numpy; ValueError when the length is wrong or one lies outside 0 .. num_class - 1."""
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    if labels.shape[0] != count:
        raise ValueError('affinity_ops: %d %s labels for %d feature rows' % (labels.shape[0], name, count))
    if count and (labels.min() < 0 or labels.max() >= num_class):
        raise ValueError('affinity_ops: a %s label outside 0 .. %d (found %d .. %d)'
                         % (name, num_class - 1, labels.min(), labels.max()))
    return labels


def _require_feats(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('affinity_ops: %s must be a tensor on the GPU (there is no CPU path)' % name)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise RuntimeError('affinity_ops: %s must be a 2-D fp32 tensor' % name)
    return t.detach().contiguous()


def _dev(t, device, dtype):
    """A host tensor -> device through pinned staging (datasets._dev: the host does not wait for the stream)."""
    return t.to(dtype).contiguous().pin_memory().to(device, non_blocking=True)


def _draws(D, K, n, epochs, init, perms):
    """(W0 (K, D) fp32, b0 (K,) fp32, perms (epochs, n) int64) on the host: given, else drawn -- the init first."""
    if init is None:
        init = draw_init(D, K)
    W0, b0 = (torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).detach().cpu().float() for v in init)
    if tuple(W0.shape) != (K, D) or tuple(b0.shape) != (K,):
        raise ValueError('affinity_ops: init must be (W (%d, %d), b (%d,))' % (K, D, K))
    if perms is None or epochs == 0:
        perms = draw_perms(n, epochs)
    else:
        perms = torch.as_tensor(np.asarray([np.asarray(p) for p in perms]) if not isinstance(perms, torch.Tensor)
                                else perms).detach().cpu().long().reshape(epochs, -1)
        if perms.shape[1] != n or (epochs and not torch.equal(perms.sort(1).values,
                                                              torch.arange(n).expand(epochs, n))):
            raise ValueError('affinity_ops: perms must hold one permutation of 0 .. %d per epoch' % (n - 1))
    return W0, b0, perms


def train_linear_probe(train_feats, train_labels, num_class, epochs=300, batch=BATCH, lr=1e-3, weight_decay=0.05,
                       t_max=300, init=None, perms=None):
    """The reference's training loop (runner_finetune.py:1203-1242) on pdae_linear_probe_train.

    train_feats (n, D) fp32 on the device; train_labels (n,) host array or tensor, 0 .. num_class - 1; init: (W (K, D),
    b (K,)) in place of the nn.Linear draw; perms: (epochs, n) in place of the randperm draws.
    -> (W (K, D), b (K,)) fp32 on the device.  The host only enqueues: nothing is read back."""
    K = int(num_class)
    n_rows = int(train_feats.shape[0]) if hasattr(train_feats, 'shape') and len(train_feats.shape) == 2 else 0
    labels = _host_labels(train_labels, n_rows, K, 'train')            # before anything touches the library
    X = _require_feats(train_feats, 'train_feats')
    n, D = X.shape
    if int(batch) != BATCH:
        raise NotImplementedError('affinity_ops: the kernels train batches of %d (PDAE_AFFINITY=torch takes others)' % BATCH)
    epochs = int(epochs)
    handle = _lib.lib()
    # K < 2, K above the cap, D < 1: raises here, before anything is launched
    _lib._check(handle, 'pdae_linear_probe_supported', handle.pdae_linear_probe_supported(n, D, X.stride(0), K))
    W0, b0, perms = _draws(D, K, n, epochs, init, perms)
    dev = X.device
    W, b = _dev(W0, dev, torch.float32), _dev(b0, dev, torch.float32)
    if epochs == 0 or n // BATCH == 0:
        return W, b
    perm_d = _dev(perms, dev, torch.int32)
    labels_d = _dev(torch.from_numpy(labels), dev, torch.int32)
    lrs = (ctypes.c_double * epochs)(*cosine_lrs(float(lr), t_max, epochs))
    ws = torch.empty(int(handle.pdae_linear_probe_workspace(D, K)), device=dev, dtype=torch.float32)
    _lib.call('pdae_linear_probe_train', X, n, D, X.stride(0), K, epochs, _lib.ptr(X), _lib.ptr(labels_d), _lib.ptr(perm_d),
              _lib.ptr(W), _lib.ptr(b), lrs, BETAS[0], BETAS[1], EPS, float(weight_decay), _lib.ptr(ws))
    return W, b


def evaluate(W, b, test_feats, test_labels, return_logits=False):
    """The reference's test pass (runner_finetune.py:1245-1269) on pdae_linear_probe_eval -> (accuracy as a fraction, mean
    cross-entropy) [, logits (m, K) on the device].  The reference adds loss.item() * batch over batches of 64; this is
    the fp64 sum of the per-row fp32 losses divided on the host: the same sum up to the fp32 rounding of each batch
    mean."""
    K = int(W.shape[0])
    m_rows = int(test_feats.shape[0]) if hasattr(test_feats, 'shape') and len(test_feats.shape) == 2 else 0
    labels = _host_labels(test_labels, m_rows, K, 'test')
    X = _require_feats(test_feats, 'test_feats')
    m, D = X.shape
    W, b = _lib.require(W.detach(), 'W', dim=2), _lib.require(b.detach(), 'b', dim=1)
    if W.shape[1] != D or b.shape[0] != K:
        raise ValueError('affinity_ops: W %r, b %r for features of width %d' % (tuple(W.shape), tuple(b.shape), D))
    if m == 0:
        raise ValueError('affinity_ops: no test rows')
    handle = _lib.lib()
    _lib._check(handle, 'pdae_linear_probe_supported', handle.pdae_linear_probe_supported(m, D, X.stride(0), K))
    dev = X.device
    labels_d = _dev(torch.from_numpy(labels), dev, torch.int32)
    row_loss = torch.empty(m, device=dev, dtype=torch.float32)
    row_pred = torch.empty(m, device=dev, dtype=torch.int32)
    logits = torch.empty((m, K), device=dev, dtype=torch.float32) if return_logits else None
    loss_sum = torch.empty(1, device=dev, dtype=torch.float64)
    correct = torch.empty(1, device=dev, dtype=torch.int32)
    _lib.call('pdae_linear_probe_eval', X, m, D, X.stride(0), K, _lib.ptr(X), _lib.ptr(labels_d), _lib.ptr(W), _lib.ptr(b),
              _lib.ptr(row_loss), _lib.ptr(row_pred), _lib.ptr(logits), _lib.ptr(loss_sum), _lib.ptr(correct))
    acc, loss = int(correct.item()) / m, float(loss_sum.item()) / m
    return (acc, loss, logits) if return_logits else (acc, loss)


def torch_train_linear_probe(train_feats, train_labels, num_class, epochs=300, batch=BATCH, lr=1e-3, weight_decay=0.05,
                             t_max=300, init=None, perms=None):
    """PDAE_AFFINITY=torch: the reference's own training loop (runner_finetune.py:1203-1242) as framework ops on the
    features' device, from the shared draws -> the trained nn.Linear."""
    n, D = train_feats.shape
    K = int(num_class)
    dev = train_feats.device
    tr_l = torch.from_numpy(_host_labels(train_labels, n, K, 'train')).to(dev)
    W0, b0, perms = _draws(D, K, n, int(epochs), init, perms)
    net = torch.nn.Linear(D, K)
    with torch.no_grad():
        net.weight.copy_(W0)
        net.bias.copy_(b0)
    net = net.to(dev)
    criterion = torch.nn.CrossEntropyLoss()
    optimizer = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=weight_decay)
    schedule = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=t_max)
    for epoch in range(int(epochs)):
        r = perms[epoch].to(dev)
        feats, labels = train_feats[r], tr_l[r]
        for i in range(n // batch):
            optimizer.zero_grad()
            loss = criterion(net(feats[i * batch:(i + 1) * batch]), labels[i * batch:(i + 1) * batch])
            loss.backward()
            optimizer.step()
        schedule.step()
    return net


def torch_evaluate(net, test_feats, test_labels, batch=BATCH):
    """The reference's test pass (runner_finetune.py:1245-1269) as it stands: loss.item() * rows added over batches of 64
    with a short last one -> (accuracy as a fraction, mean cross-entropy)."""
    m = test_feats.shape[0]
    te_l = torch.from_numpy(_host_labels(test_labels, m, net.out_features, 'test')).to(test_feats.device)
    criterion = torch.nn.CrossEntropyLoss()
    loss_sum, correct = 0.0, 0
    with torch.no_grad():
        for i in range(0, m, batch):
            out, lab = net(test_feats[i:i + batch]), te_l[i:i + batch]
            loss_sum += criterion(out, lab).item() * out.shape[0]
            correct += (out.argmax(1) == lab).sum().item()
    return correct / m, loss_sum / m


def task_affinity_loss(train_feats, train_labels, test_feats, test_labels):
    """The protocol's two numbers from the features: num_class = max(test labels) + 1 (runner_finetune.py:1199), the probe
    trained with the reference's recipe, -> (accuracy as a fraction, mean test cross-entropy); on the kernels
    (PDAE_AFFINITY=hip) or as framework ops (PDAE_AFFINITY=torch)."""
    name = backend()
    te = test_labels.detach().cpu().numpy() if isinstance(test_labels, torch.Tensor) else np.asarray(test_labels)
    if te.size == 0:
        raise ValueError('affinity_ops: no test rows')
    num_class = int(te.max()) + 1
    # (both label sets are checked before the first draw and the first launch)
    _host_labels(train_labels, train_feats.shape[0], num_class, 'train')
    _host_labels(te, test_feats.shape[0], num_class, 'test')
    if name == 'torch':
        return torch_evaluate(torch_train_linear_probe(train_feats, train_labels, num_class), test_feats, te)
    W, b = train_linear_probe(train_feats, train_labels, num_class)
    return evaluate(W, b, test_feats, te)
