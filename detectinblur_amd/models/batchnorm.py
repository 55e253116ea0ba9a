"""`BatchNorm2d` with the reference's test-time "mode one" (reference models/batchnorm.py:159-184; `evaluate.py
--mode_one_norm`): every batch-norm layer normalises with its running statistics mixed with the statistics of the batch it
sees, whatever `self.training` says,

    mean = f * running_mean + g * mean_b,   var = f * running_var + g * var_b,   f = n / (n + 1),  g = 1 / (n + 1)

with n = num_batches_tracked and var_b the biased variance over N x H x W -- zero padding of the batched images included.
Two ways to the same values:

  * HIP (include/dib.h: dib_bn_mode_one_nhwc): a CUDA fp32 channels-last tensor with C % 4 == 0 and no autograd graph to
    build -- partial Welford statistics, the mix and the fused scale / shift (+ residual) (+ ReLU) pass, three launches;
  * torch: everything else (CPU, planar tensors, gradients), a line-for-line restatement of the reference's forward, bit for
    bit its values (tests/test_mode_one_norm.py).

`acclimation_mode` (reference models/batchnorm.py:142-157; `evaluate.py --acclimate_norm`) is the online form: the layer first
folds the statistics of the batch it sees into its running statistics -- F.batch_norm(..., training=True, a) with a the momentum
or, with `momentum = None` in training mode, 1 / num_batches_tracked after its bump -- and then normalises with the updated
running statistics.  It wins over `mode_one` where both are set, as in the reference.  The same two ways:

  * HIP (dib_bn_acclimate_nhwc): under the conditions above, with the running statistics and the counter updated IN PLACE on the
    device (a captured graph's replays and the pipelined loop carry the state; nothing is read on the host).  A training layer's
    counter must therefore be on the device; one value per channel goes to the torch path, which raises torch's error;
  * torch: the reference's forward, statement for statement, `self.num_batches_tracked = self.num_batches_tracked + 1` included --
    a rebinding that a captured graph must never see, so this path refuses to run under capture.

With both flags off the module is `torch.nn.BatchNorm2d`.  `last_path` records which of the two ran last ("hip" / "torch"), for
tests and A/B runs; the switch for those is backbone.FUSE_TEST_TIME_BN.
"""
import torch
import torch.nn.functional as F
from torch import nn


class BatchNorm2d(nn.BatchNorm2d):
    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device=device, dtype=dtype)
        self.mode_one = False
        self.acclimation_mode = False
        self.last_path = None

    # ---- which path ------------------------------------------------------------------------------------------------------------
    def _hip_state_ok(self, dev):
        """Whether this layer, as it is configured and where its state lives, may take the HIP path for inputs on `dev`: every
        condition of that path that does not depend on the input.  `_hip_ok` adds the input's; utils.acclimation_on_device asks
        this alone, before any input exists."""
        from . import backbone
        if not (backbone.FUSE_TEST_TIME_BN and dev.type == "cuda"):
            return False
        if self.running_mean is None or self.running_var is None or (self.training and not self.track_running_stats):
            return False
        nbt = self.num_batches_tracked
        if self.training and self.track_running_stats and nbt is not None:
            # the reference bumps num_batches_tracked first: mode one's torch path does that; the acclimation kernel does it itself,
            # in place, on a counter that lives on the device
            if not (self.acclimation_mode and nbt.device == dev):
                return False
        if nbt is not None and not (nbt.dtype == torch.int64 and nbt.numel() == 1 and (nbt.device == dev or nbt.device.type == "cpu")):
            return False
        if self.acclimation_mode and self.momentum is not None and not (0.0 <= float(self.momentum) <= 1.0):
            return False
        for t in (self.weight, self.bias, self.running_mean, self.running_var):
            if t is not None and not (t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
                return False
        return not (torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in (self.weight, self.bias)))

    def _hip_ok(self, x, residual=None):
        if not (x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] % 4 == 0 and x.numel() > 0
                and x.is_contiguous(memory_format=torch.channels_last) and not (x.data_ptr() & 15) and self._hip_state_ok(x.device)):
            return False
        if self.acclimation_mode and x.shape[0] * x.shape[2] * x.shape[3] < 2:
            return False                # torch raises for one value per channel in training mode: the torch path shows that error
        if torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)):
            return False
        return residual is None or (residual.shape == x.shape and residual.dtype == torch.float32 and residual.device == x.device
                                    and residual.is_contiguous(memory_format=torch.channels_last) and not (residual.data_ptr() & 15))

    def _hip_method(self):
        """The HIP method of the layer's mode: acclimation wins over mode one, as in the reference; None with both off."""
        if self.acclimation_mode:
            return self._acclimate_hip_
        return self._mode_one_hip_ if self.mode_one else None

    # ---- the two paths ---------------------------------------------------------------------------------------------------------
    def _hip_call_(self, entry, middle, x, residual, relu, stats):
        """x = act(bn(x) (+ residual)) in place through `entry` (dib_bn_mode_one_nhwc or dib_bn_acclimate_nhwc); `middle`: what
        their argument lists do not share, between running_var and eps."""
        from .. import _lib
        N, C, H, W = x.shape
        npix = N * H * W
        l = _lib.lib()
        nbytes = l.dib_bn_mode_one_workspace_bytes(npix, C)
        ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=x.device)      # the caching allocator (a graph's pool under capture)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        _lib.check(getattr(l, entry)(x.data_ptr(), ptr(residual), npix, C, ptr(self.weight), ptr(self.bias), self.running_mean.data_ptr(),
                                     self.running_var.data_ptr(), *middle, float(self.eps), int(bool(relu)), ws.data_ptr(), ws.numel() * 4,
                                     ptr(stats), _lib.stream_of(x)))
        self.last_path = "hip"
        return x

    def _mode_one_hip_(self, x, residual=None, relu=False, stats=None):
        """x = act(bn(x) (+ residual)) in place (dib_bn_mode_one_nhwc).  `stats`: a [2, C] fp32 CUDA tensor that receives the mixed
        mean and variance."""
        nbt = self.num_batches_tracked
        if nbt is None:
            nb_dev, nb_host = None, 0
        elif nbt.is_cuda:
            nb_dev, nb_host = nbt.data_ptr(), 0          # read on the device: no host synchronisation
        else:
            nb_dev, nb_host = None, int(nbt)             # a CPU tensor: read here (a captured graph keeps this value)
        return self._hip_call_("dib_bn_mode_one_nhwc", (nb_dev, nb_host), x, residual, relu, stats)

    def _mode_one_torch(self, input):
        """reference models/batchnorm.py:97-184 for mode_one (acclimation off), statement for statement."""
        if self.momentum is None:
            exponential_average_factor = 0.0
        else:
            exponential_average_factor = self.momentum
        if self.training and self.track_running_stats:
            if self.num_batches_tracked is not None:
                self.num_batches_tracked = self.num_batches_tracked + 1
                if self.momentum is None:
                    exponential_average_factor = 1.0 / float(self.num_batches_tracked)
                else:
                    exponential_average_factor = self.momentum
        if self.training:
            bn_training = True
        else:
            bn_training = (self.running_mean is None) and (self.running_var is None)
        passed_running_mean = self.running_mean if not self.training or self.track_running_stats else None
        passed_running_var = self.running_var if not self.training or self.track_running_stats else None
        self.last_path = "torch"
        if passed_running_mean is None:
            return F.batch_norm(input, passed_running_mean, passed_running_var, self.weight, self.bias, bn_training,
                                exponential_average_factor, self.eps)
        input_var = input.permute([1, 0, 2, 3]).reshape(input.shape[1], input.shape[0] * input.shape[2] * input.shape[3]).var(axis=1, unbiased=False)
        input_mean = input.mean(axis=3).mean(axis=2).mean(0)
        source_stat_factor = torch.true_divide(self.num_batches_tracked, (self.num_batches_tracked + torch.tensor(1)))
        batch_stat_factor = torch.true_divide(torch.tensor(1), (self.num_batches_tracked + torch.tensor(1)))
        mean_to_use = source_stat_factor * passed_running_mean + batch_stat_factor * input_mean
        var_to_use = source_stat_factor * passed_running_var + batch_stat_factor * input_var
        return F.batch_norm(input, mean_to_use, var_to_use, self.weight, self.bias, False, 0.0, self.eps)

    def _acclimate_hip_(self, x, residual=None, relu=False, stats=None):
        """x = act(bn(x) (+ residual)) in place with running_mean, running_var and (training mode) num_batches_tracked updated in
        place on the device (dib_bn_acclimate_nhwc).  `stats`: a [4, C] fp32 CUDA tensor that receives the batch mean, the unbiased
        batch variance and the updated running pair."""
        nbt = self.num_batches_tracked
        bump = bool(self.training and self.track_running_stats and nbt is not None)
        nb_dev = nbt.data_ptr() if nbt is not None and nbt.is_cuda else None
        momentum = -1.0 if self.momentum is None else float(self.momentum)
        return self._hip_call_("dib_bn_acclimate_nhwc", (nb_dev, int(bump), momentum), x, residual, relu, stats)

    def _acclimate_torch(self, input):
        """reference models/batchnorm.py:105-157 for acclimation_mode, statement for statement."""
        if input.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("BatchNorm2d: the torch path of acclimation_mode rebinds num_batches_tracked and cannot be captured into a graph")
        self._check_input_dim(input)
        if self.momentum is None:
            exponential_average_factor = 0.0
        else:
            exponential_average_factor = self.momentum
        if self.training and self.track_running_stats:
            if self.num_batches_tracked is not None:
                self.num_batches_tracked = self.num_batches_tracked + 1
                if self.momentum is None:
                    exponential_average_factor = 1.0 / float(self.num_batches_tracked)
                else:
                    exponential_average_factor = self.momentum
        passed_running_mean = self.running_mean if not self.training or self.track_running_stats else None
        passed_running_var = self.running_var if not self.training or self.track_running_stats else None
        self.last_path = "torch"
        # two runs through batch_norm: one takes the batch's statistics and updates the running ones (training set to True), the
        # other computes the output from the running statistics so far (training set to False)
        _ = F.batch_norm(input, passed_running_mean, passed_running_var, self.weight, self.bias, True, exponential_average_factor, self.eps)
        output = F.batch_norm(input, passed_running_mean, passed_running_var, self.weight, self.bias, False, 0.0, self.eps)
        return output

    # ---- entry points ----------------------------------------------------------------------------------------------------------
    def forward(self, input):
        hip = self._hip_method()
        if hip is None:
            return super().forward(input)
        if self._hip_ok(input):
            return hip(input.clone(memory_format=torch.channels_last))
        return self._acclimate_torch(input) if self.acclimation_mode else self._mode_one_torch(input)

    def forward_fused_(self, x, residual=None, relu=False):
        """act(self(x) (+ residual)), in place on x where the HIP path applies (x: a fresh convolution output nothing else holds)."""
        hip = self._hip_method()
        if hip is not None and self._hip_ok(x, residual):
            return hip(x, residual, relu)
        y = self(x)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y
