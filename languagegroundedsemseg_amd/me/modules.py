"""Module surface: MinkowskiConvolution[Transpose], MinkowskiBatchNorm, MinkowskiSyncBatchNorm,
MinkowskiReLU, MinkowskiNetwork ... with the constructor signatures, parameter names and shapes the
reference relies on:
  kernel [K,Cin,Cout] ([Cin,Cout] for 1x1 stride 1), bias [1,Cout]     common.py:195-203,228-236
  MinkowskiBatchNorm.bn = nn.BatchNorm1d                               common.py:19, resnet.py:80-82
so released checkpoints' state-dict keys/shapes load (lib/utils.py:17-45).
"""
import math
from enum import Enum

import torch
import torch.nn as nn

from . import deferred as _deferred
from .core import SparseTensor, get_backend
from .kernel import KernelGenerator, RegionType, conv_relation, convert_to_int_list, supported_convs_text
from .host import AffineSink, WeightSink, param_event, relu_mode_of, row_stride, side_wgrads_issued, wgrad_placement


class MinkowskiModuleBase(nn.Module):
    pass


def _invalidate_packed():
    be = get_backend()
    if hasattr(be, "invalidate_packed_weights"):
        be.invalidate_packed_weights()


def _invalidate_packed_hook(module, incompatible_keys):
    """load_state_dict post-hook (a module-level function: hooks are pickled with the module)"""
    _invalidate_packed()


class MinkowskiNetwork(nn.Module):
    """models/model.py:4-16 subclasses this and stores D."""

    def __init__(self, D):
        super().__init__()
        self.D = D


# ------------------------------------------------------------------------------------------ convolution
def conv_weight_grad(kmap, feats, gout, transposed, kparam, kshape, kdtype):
    """Weight gradient of one convolution.  When the kernel parameter owns a bucket slot the gradient is written straight
    into it ON A SIDE STREAM (off the backward critical path dgrad -> BN -> dgrad ...; both kernels are latency-bound, so
    running them concurrently fills the machine) and the slot view is returned for autograd to adopt as `.grad`;
    host.wgrad_placement has the exceptions."""
    sink = WeightSink(kparam)
    backend = get_backend()
    where = wgrad_placement(sink.adopted and gout.is_cuda and hasattr(backend, "side_stream"), feats.shape[1], gout.shape[1],
                            gout.shape[0], getattr(kmap.mgr, "inline_wgrad", False))
    if where == "plain":
        return kmap.conv_wgrad(feats, gout, transposed).reshape(kshape).to(kdtype)
    view, = sink.bufs
    if where == "inline":
        kmap.conv_wgrad(feats, gout, transposed, out=view.view(kmap.K, -1, kshape[-1]))
    elif where == "side":
        dev = gout.device
        side = backend.side_stream(dev)
        fork = backend.fork_event(dev)
        fork.record(backend.current_stream(dev))             # feats / gout are ready
        side.wait_event(fork)
        kmap.conv_wgrad(feats, gout, transposed, out=view.view(kmap.K, -1, kshape[-1]), stream=side)
        param_event(kparam).record(side)
        side_wgrads_issued(side, (kparam,), (feats, gout))
    return view                                              # consumers wait for the side stream in BucketedDDP


def _bias_grad(gout):
    """column sums of the output gradient in fp32.  On the engine: the BatchNorm statistics reduction (two launches at the
    streaming rate: per-block sums about a pivot, folded in double in a fixed order) read as mean x count -- torch's reduction
    of the [1.2 M, 200] bf16 gradient of the classifier took 190 us of the step."""
    backend = get_backend()
    c = gout.shape[1]
    if hasattr(backend, "bn_stats") and gout.is_cuda and gout.is_contiguous() and gout.shape[0] > 0 and \
            c % (8 if gout.dtype == torch.bfloat16 else 4) == 0 and gout.dtype in (torch.bfloat16, torch.float32):
        rec = backend.bn_stats(gout)                           # [mean | M2 | count]
        return (rec[:c] * rec[2 * c]).view(1, c)
    return gout.sum(0, keepdim=True, dtype=torch.float32)      # fp32 accumulation without an fp32 copy of gout


class MinkowskiConvolutionFunction(torch.autograd.Function):
    """out = conv(in) over a cached kernel map; backward = dgrad + wgrad (conv_weight_grad) (+ bias grad) on the same map."""

    @staticmethod
    def forward(ctx, feats, kernel, bias, kmap, transposed, bn_pivot=None, want_bn_stats=False, pack_cache=None):
        ctx.kmap, ctx.transposed, ctx.has_bias = kmap, transposed, bias is not None
        ctx.pack_cache = pack_cache
        kw = {"pack_cache": pack_cache} if pack_cache is not None else {}
        ctx.kshape = kernel.shape
        ctx.kparam = kernel if isinstance(kernel, torch.nn.Parameter) else None
        ctx.save_for_backward(feats, kernel)
        if want_bn_stats:
            # the conv epilogue also emits per-tile sum / sum-of-squares of its output for the BatchNorm that follows
            out, stats = kmap.conv_forward(feats, kernel, bias, transposed, bn_pivot=bn_pivot, want_bn_stats=True, **kw)
            ctx.bn_stats = stats                 # picked up by MinkowskiConvolutionBase.forward (not a graph output)
            return out
        return kmap.conv_forward(feats, kernel, bias, transposed, **kw)

    @staticmethod
    def backward(ctx, gout):
        feats, kernel = ctx.saved_tensors
        gout = gout.contiguous()
        gin = gw = gb = None
        if ctx.needs_input_grad[1]:
            gw = conv_weight_grad(ctx.kmap, feats, gout, ctx.transposed, ctx.kparam, ctx.kshape, kernel.dtype)
        if ctx.needs_input_grad[0]:
            if getattr(ctx, "pack_cache", None) is not None:
                gin = ctx.kmap.conv_dgrad(gout, kernel, ctx.transposed, pack_cache=ctx.pack_cache)
            else:
                gin = ctx.kmap.conv_dgrad(gout, kernel, ctx.transposed)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _bias_grad(gout)
        return gin, gw, gb, None, None, None, None, None


MinkowskiConvolutionTransposeFunction = MinkowskiConvolutionFunction


class _StatsHolder:
    stats = None


class _ConvStatsFunction(MinkowskiConvolutionFunction):
    """MinkowskiConvolutionFunction whose forward also asks the kernel for the next norm's statistics (side output)."""

    @staticmethod
    def forward(ctx, feats, kernel, kmap, transposed, bn_pivot, holder, pack_cache=None):
        out = MinkowskiConvolutionFunction.forward(ctx, feats, kernel, None, kmap, transposed, bn_pivot, True, pack_cache)
        holder.stats = ctx.bn_stats
        ctx.bn_stats = None
        return out

    @staticmethod
    def backward(ctx, gout):
        gin, gw = MinkowskiConvolutionFunction.backward(ctx, gout)[:2]
        return gin, gw, None, None, None, None, None


def _conv_with_stats(feats, kernel, kmap, transposed, pivot, holder, pack_cache=None):
    return _ConvStatsFunction.apply(feats, kernel, kmap, transposed, pivot, holder, pack_cache)


class MinkowskiConvolutionBase(MinkowskiModuleBase):
    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                 is_transpose=False, expand_coordinates=False, convolution_mode=None, dimension=-1):
        super().__init__()
        assert dimension > 0, "dimension must be a positive integer"
        if kernel_generator is None:
            kernel_generator = KernelGenerator(kernel_size=kernel_size, stride=stride, dilation=dilation,
                                               expand_coordinates=expand_coordinates, dimension=dimension)
        self.is_transpose = is_transpose
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_generator = kernel_generator
        self.dimension = dimension
        self.use_mm = False
        self.kernel_size = kernel_generator.kernel_size
        self.stride = kernel_generator.kernel_stride
        self.dilation = kernel_generator.kernel_dilation
        if kernel_generator.region_type != RegionType.HYPER_CUBE:
            raise NotImplementedError("only HYPER_CUBE regions are part of the D=3 model family")
        if len(set(self.kernel_size)) != 1 or len(set(self.stride)) != 1 or len(set(self.dilation)) != 1:
            raise NotImplementedError("anisotropic kernels / strides / dilations are not supported on D=3")
        ks, st, dil = self.kernel_size[0], self.stride[0], self.dilation[0]
        if conv_relation(ks, st, dil) is None:
            raise NotImplementedError("(kernel_size, stride, dilation) = (%d, %d, %d) is not supported: the supported set is %s" % (
                ks, st, dil, supported_convs_text()))
        self.kernel_volume = kernel_generator.kernel_volume
        if self.kernel_volume == 1 and st == 1:
            self.use_mm = True
            kshape = (in_channels, out_channels)
        else:
            kshape = (self.kernel_volume, in_channels, out_channels)
        self._pack_cache = {}        # packed weight images of this module's launch shapes (backend_hip.PackedWeights)
        self.kernel = nn.Parameter(torch.empty(kshape, dtype=torch.float32))
        self.bias = nn.Parameter(torch.empty((1, out_channels), dtype=torch.float32)) if bias else None
        self.reset_parameters()
        # load_state_dict() copies into `.data` without bumping the parameter's version counter: drop the packed images
        self.register_load_state_dict_post_hook(_invalidate_packed_hook)

    def __getstate__(self):
        # packed weight images are a device-side cache tied to this process: never pickled / deep-copied with the module
        state = self.__dict__.copy()
        state["_pack_cache"] = {}
        return state

    def reset_parameters(self, is_transpose=None):
        is_transpose = self.is_transpose if is_transpose is None else is_transpose
        with torch.no_grad():
            n = (self.out_channels if is_transpose else self.in_channels) * self.kernel_volume
            stdv = 1.0 / math.sqrt(n)
            self.kernel.data.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.data.uniform_(-stdv, stdv)
        _invalidate_packed()      # `.data` writes are invisible to the version counter the packed-image cache keys on

    def forward(self, input, coordinates=None, bn=None):
        """Standard call: `conv(x)` records the convolution (me/deferred.py) and returns a tensor whose features are pending; the
        coordinate map / kernel map it needs are requested now (built on the engine's map stream).
        `bn` (extension, used by the executor and by tests): the MinkowskiBatchNorm this output goes to next; runs immediately."""
        assert isinstance(input, SparseTensor)
        nch = input._nch()
        assert nch == self.in_channels, "Channel size mismatch %d != %d" % (nch, self.in_channels)
        if bn is None and _deferred.ENABLED:
            return _deferred.record_conv(self, input, self._resolve(input))
        return self._forward_now(input, bn)

    def _resolve(self, input):
        """-> (output coordinate map key, kernel map, transposed)"""
        mgr = input.coordinate_manager
        ks, st, dil = self.kernel_size[0], self.stride[0], self.dilation[0]
        in_key = input.coordinate_map_key
        if not self.is_transpose:
            out_key = in_key if st == 1 else mgr.stride(in_key, st)
            return out_key, mgr.kernel_map_handle(in_key, out_key, ks, dil), False
        out_key = in_key if st == 1 else mgr.finer_key(in_key)
        # the transposed conv reuses the forward map of the matching strided conv, in/out swapped
        return out_key, mgr.kernel_map_handle(out_key, in_key, ks, dil), True

    def _forward_now(self, input, bn=None, resolved=None, out=None):
        """run the convolution.  `bn`: in training the conv epilogue may also produce that norm's batch statistics (pivoted on its
        running mean; off by default, CONV_BN_STATS) and hand them over on the output tensor.  `out`: the pending tensor to fill."""
        mgr = input.coordinate_manager
        out_key, kmap, transposed = resolved if resolved is not None else self._resolve(input)
        x = input.F
        stats = None
        want = (bn is not None and getattr(get_backend(), "conv_bn_stats", False) and bn.bn.training and bn.bn.affine and x.is_cuda
                and self.bias is None
                and get_backend().want_conv_bn_stats(mgr.size(out_key), self.out_channels, x.element_size()))
        if want:
            pivot = bn.bn.running_mean if bn.bn.track_running_stats else None
            holder = _StatsHolder()
            y = _conv_with_stats(x, self.kernel, kmap, transposed, pivot, holder, self._cache_for(x))
            stats = holder.stats                   # (partials, pivot) or None
        else:
            y = MinkowskiConvolutionFunction.apply(x, self.kernel, self.bias, kmap, transposed, None, False, self._cache_for(x))
        if out is None:
            out = SparseTensor(y, coordinate_map_key=out_key, coordinate_manager=mgr)
        else:
            out._F, out._op = y, None
        out._bn_stats = stats
        return out

    def _cache_for(self, feats):
        """packed-image cache of this module, only on the HIP backend with an fp32 master weight"""
        if not feats.is_cuda or not getattr(get_backend(), "weights_updated", None) or self.kernel.dtype != torch.float32:
            return None
        return self._pack_cache

    def __repr__(self):
        return "%s(in=%d, out=%d, kernel_size=%s, stride=%s, dilation=%s)" % (
            self.__class__.__name__, self.in_channels, self.out_channels, self.kernel_size, self.stride, self.dilation)


class MinkowskiConvolution(MinkowskiConvolutionBase):
    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                 expand_coordinates=False, convolution_mode=None, dimension=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, kernel_generator,
                         is_transpose=False, expand_coordinates=expand_coordinates, convolution_mode=convolution_mode,
                         dimension=dimension)


class MinkowskiConvolutionTranspose(MinkowskiConvolutionBase):
    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                 expand_coordinates=False, convolution_mode=None, dimension=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, kernel_generator,
                         is_transpose=True, expand_coordinates=expand_coordinates, convolution_mode=convolution_mode,
                         dimension=dimension)


# ------------------------------------------------------------------------------------------ normalisation
def bn_fwd(be, x, bn, g, b, residual, relu, conv_stats=None, sync=(False, None), out_into=None):
    """training-mode y = relu?(BN(x) (+ residual)) of the nn.BatchNorm1d `bn` with affine g, b -> y, stats, inv_n.  sync = (True,
    process group): the statistics are exchanged across the group's ranks (ddp.sync_bn_forward) and inv_n is the device scalar
    1 / global rows, else None.  conv_stats: (partials, pivot) from the producing conv's epilogue; out_into: the _CatSlot y goes to."""
    if conv_stats is not None and (conv_stats[1] is not None) != (bn.running_mean is not None):
        conv_stats = None                                  # pivot convention mismatch (cannot happen for the conv's own bn)
    out = (out_into.buf, out_into.off) if out_into is not None else None
    if sync[0]:
        from ..ddp import sync_bn_forward
        return sync_bn_forward(be, x, g, b, residual, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum,
                               relu, sync[1], conv_stats, out)
    nbt = bn.num_batches_tracked if be.bn_counts_batches else None        # (else the caller has counted the batch)
    return be.bn_forward(x, g, b, bn.eps, bn.momentum, bn.running_mean, bn.running_var, residual, relu, nbt, conv_stats=conv_stats,
                         out_into=out) + (None,)


def bn_bwd(be, x, y, dy, g, b, gp, bp, stats, relu_mode, want_res, need, sync=(False, None), inv_n=None):
    """-> dx, dres, d gamma, d beta: the last two as bucket-slot views when the parameters gp / bp own slots, else cast to g's dtype
    (None when not `need`ed).  dy / y may be column slices of a concat buffer: the engine reads them in place."""
    sink = AffineSink(gp, bp, x.shape[1], x.device)
    if sync[0]:
        from ..ddp import sync_bn_backward
        dx, dres = sync_bn_backward(be, x, y, dy, g, b, stats, inv_n, relu_mode, want_res, sync[1], sink)
    else:
        dx, dres = be.bn_backward(x, y, dy, g, b, stats, relu_mode, want_res, *sink.bufs)[:2]
    return (dx, dres) + sink.returned(g.dtype, need)


class BatchNormFunction(torch.autograd.Function):
    """y = relu?(BN(x) (+ residual)) with batch statistics -- of this rank, or of every rank of sync's process group -- as one
    node around bn_fwd / bn_bwd (the whole-block node of me/block.py calls the same two functions)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, bn, relu, backend, sync=(False, None), conv_stats=None, out_into=None):
        y, stats, inv_n = bn_fwd(backend, x, bn, gamma, beta, residual, relu, conv_stats, sync, out_into)
        ctx.gparam = gamma if isinstance(gamma, torch.nn.Parameter) else None
        ctx.bparam = beta if isinstance(beta, torch.nn.Parameter) else None
        ctx.backend, ctx.sync, ctx.has_res = backend, sync, residual is not None
        ctx.relu_mode = relu_mode_of(relu, ctx.has_res)
        saved = (x, gamma, beta, stats) + ((y,) if ctx.relu_mode == 1 else ()) + ((inv_n,) if inv_n is not None else ())
        ctx.save_for_backward(*saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        x, gamma, beta, stats = saved[:4]
        dx, dres, dgamma, dbeta = bn_bwd(ctx.backend, x, saved[4] if ctx.relu_mode == 1 else None, dy, gamma, beta, ctx.gparam,
                                         ctx.bparam, stats, ctx.relu_mode, ctx.has_res and ctx.needs_input_grad[3], True, ctx.sync,
                                         saved[-1] if ctx.sync[0] else None)
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None


class _CatSlot:
    """where a norm writes its output for a zero-copy ME.cat: column offset `off` of the [N, C_total] concat buffer `buf`
    (a plain Python object on purpose: autograd must not see the buffer as a tensor input of the norm)"""

    partner = None       # the skip tensor whose features were COPIED into the right-hand columns (half-copy concat)

    def __init__(self, buf, off, width):
        self.buf, self.off, self.width = buf, off, width


def _cat_buffer(x, left, right):
    """a fresh [N, left + right] concat buffer in x's dtype whose two column halves the engine can address in place
    (host.row_stride), or None"""
    buf = torch.empty((x.shape[0], left + right), dtype=x.dtype, device=x.device)
    return buf if row_stride(buf[:, :left], left) and row_stride(buf[:, left:], right) else None


class EvalBatchNormFunction(torch.autograd.Function):
    """eval-mode BatchNorm (running statistics) (+ residual) (+ ReLU) on the engine's apply kernels: forward =
    lgs_bn_apply with stats = [running_mean | 1/sqrt(running_var + eps)]; backward (frozen statistics: fine-tuning with
    BN in eval mode) = lgs_bn_backward_reduce for d gamma / d beta and lgs_bn_backward_apply with zero batch sums."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, stats, relu, backend):
        y = backend.bn_apply(x, gamma, beta, stats, residual, relu)
        ctx.backend, ctx.has_res = backend, residual is not None
        ctx.relu_mode = relu_mode_of(relu, ctx.has_res)
        ctx.save_for_backward(x, gamma, beta, stats, y if ctx.relu_mode == 1 else x.new_empty(0))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, stats, y = ctx.saved_tensors
        dy = dy.contiguous()
        yy = y if ctx.relu_mode == 1 else None
        c = x.shape[1]
        sums = ctx.backend.bn_backward_reduce(x, yy, dy, gamma, beta, stats, ctx.relu_mode)
        zero = torch.zeros_like(sums)
        dx, dres = ctx.backend.bn_backward_apply(x, yy, dy, gamma, beta, stats, zero, 0.0, ctx.relu_mode,
                                                 ctx.has_res and ctx.needs_input_grad[3])
        return dx, sums[c:].to(gamma.dtype), sums[:c].to(gamma.dtype), dres, None, None, None


class MinkowskiBatchNorm(nn.Module):
    """`.bn` is a plain nn.BatchNorm1d so state-dict keys are `*.bn.{weight,bias,running_*}`."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)

    def forward(self, input, relu=False, residual=None, cat_up=0, cat_into=None):
        """Standard call: `norm(x)` records the normalisation (me/deferred.py); a following MinkowskiReLU(inplace=True) and
        `out += residual` become its epilogue, a later `me.cat` its output placement, and the whole thing runs as one kernel when
        a value is first needed.
        `relu` / `residual` / `cat_up` / `cat_into` are the executor's (and the per-op tests') way of asking for that fused kernel
        directly; with any of them the call runs immediately.  Zero-copy ME.cat(up, skip) (res16unet.py:237,247,257,267): the norm
        that produces the SKIP tensor gets cat_up = channels of the future `up` half: it allocates the [N, cat_up + C] concat buffer
        and writes its output into the right-hand columns; the norm that produces `up` gets cat_into = that skip tensor and writes
        into the left-hand columns; ME.cat then returns the buffer itself.  Both are hints: paths that cannot honour them (eval
        mode, CPU oracle backend) return ordinary tensors and ME.cat copies."""
        if _deferred.ENABLED and not relu and residual is None and not cat_up and cat_into is None:
            return _deferred.record_bn(self, input)
        return self._forward_now(input, relu, residual, cat_up, cat_into)

    def train(self, mode=True):
        if mode != self.training:
            _deferred.flush_all()          # recorded calls run with the mode they were recorded in
        return super().train(mode)

    def _forward_now(self, input, relu=False, residual=None, cat_up=0, cat_into=None, out=None):
        y, slot = self._run(input, relu, residual, cat_up, cat_into)
        if out is None:
            out = SparseTensor(y, coordinate_map_key=input.coordinate_map_key, coordinate_manager=input.coordinate_manager)
        else:
            out._F, out._op = y, None
        out._cat_slot = slot
        return out

    def _run(self, input, relu, residual, cat_up, cat_into):
        """-> (features, _CatSlot | None)"""
        bn = self.bn
        backend = get_backend()
        x = input.F
        res = residual.F if isinstance(residual, SparseTensor) else residual
        fused = hasattr(backend, "bn_forward") and bn.affine and (bn.training or not bn.track_running_stats)
        if fused:
            if bn.track_running_stats and not getattr(backend, "bn_counts_batches", False):
                bn.num_batches_tracked += 1                # (the HIP engine increments it inside the fold kernel)
            slot = self._cat_slot_for(x, cat_up, cat_into, backend) if type(self) is MinkowskiBatchNorm else None
            y = BatchNormFunction.apply(x, bn.weight, bn.bias, res, bn, relu, backend, (False, None), input._bn_stats, slot)
            return y, slot
        elif hasattr(backend, "bn_apply") and bn.affine and bn.track_running_stats and x.is_cuda:
            # eval mode on the engine too (inference / validation passes, BN frozen during fine-tuning)
            # [running_mean | 1/sqrt(running_var + eps)], rebuilt only when the running statistics were written (a frozen trunk
            # otherwise launches three tiny torch kernels per norm and step: 186 launches for Res16UNet34C)
            key = (bn.running_mean._version, bn.running_var._version, bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.eps)
            cached = getattr(self, "_eval_stats", None)
            if cached is None or cached[0] != key or cached[1].device != x.device:
                with torch.no_grad():
                    stats = torch.cat([bn.running_mean.float(), torch.rsqrt(bn.running_var.float() + bn.eps)])
                self._eval_stats = cached = (key, stats)
            stats = cached[1]
            y = EvalBatchNormFunction.apply(x, bn.weight, bn.bias, res, stats, relu, backend)
        else:   # CPU oracle backend of the tests / norms without affine parameters
            y = bn(x.float()).to(x.dtype) if x.dtype != torch.float32 else bn(x)
            if res is not None:
                y = y + res
            if relu:
                y = torch.relu(y)
        return y, None

    @staticmethod
    def _cat_slot_for(x, cat_up, cat_into, backend):
        """the column slice of a concat buffer this norm's output goes to (zero-copy ME.cat), or None"""
        if not (getattr(backend, "bn_out_into", False) and x.is_cuda):
            return None
        c = x.shape[1]
        if cat_up > 0:
            buf = _cat_buffer(x, cat_up, c)
            if buf is not None:
                return _CatSlot(buf, cat_up, c)
        if cat_into is not None:
            other = cat_into._cat_slot
            if other is not None:
                if (other.off == c and other.buf.shape[0] == x.shape[0] and other.buf.dtype == x.dtype
                        and not getattr(other, "taken", False)):
                    other.taken = True
                    return _CatSlot(other.buf, 0, c)
                return None
            # the skip tensor exists already as an ordinary tensor: this norm writes the left-hand columns of a fresh concat
            # buffer, the skip half is copied in once (me/deferred.py _cat_partner)
            if cat_into._op is None:
                sf = cat_into._F
                buf = _cat_buffer(x, c, sf.shape[1]) if (sf.is_cuda and sf.dim() == 2 and sf.shape[0] == x.shape[0]
                                                         and sf.dtype == x.dtype) else None
                if buf is not None:
                    with torch.no_grad():
                        buf[:, c:].copy_(sf)
                    slot = _CatSlot(buf, 0, c)
                    slot.partner = cat_into
                    return slot
        return None

    def __repr__(self):
        b = self.bn
        return "MinkowskiBatchNorm(%d, eps=%g, momentum=%g, affine=%s, track_running_stats=%s)" % (
            b.num_features, b.eps, b.momentum, b.affine, b.track_running_stats)


class MinkowskiSyncBatchNorm(MinkowskiBatchNorm):
    """Cross-rank batch statistics (main.py:122-123) on the engine's split BN kernels (ddp.sync_bn_forward / sync_bn_backward): every
    rank contributes one [mean | M2 | count] record to ONE all-gather per layer, the records are combined with Chan's
    parallel formula in one kernel; backward exchanges [sum dy | sum dy xhat] with ONE all-reduce of 2C floats.
    `force_sync` (class attribute, tests only) takes the collective path even in a world of one rank."""
    force_sync = False

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, process_group=None):
        super().__init__(num_features, eps, momentum, affine, track_running_stats)
        self.process_group = process_group

    def _run(self, input, relu, residual, cat_up, cat_into):
        import torch.distributed as dist
        if not (self.training and dist.is_available() and dist.is_initialized()
                and (dist.get_world_size(self.process_group) > 1 or MinkowskiSyncBatchNorm.force_sync)):
            return super()._run(input, relu, residual, cat_up, cat_into)
        from ..ddp import sync_batch_norm
        res = residual.F if isinstance(residual, SparseTensor) else residual
        backend = get_backend()
        x = input.F
        slot = self._cat_slot_for(x, cat_up, cat_into, backend) if hasattr(backend, "bn_forward_sync") else None
        y = sync_batch_norm(x, self.bn, self.process_group, residual=res, relu=relu, conv_stats=input._bn_stats, out_into=slot)
        return y, slot

    @classmethod
    def convert_sync_batchnorm(cls, module, process_group=None):
        out = module
        if isinstance(module, MinkowskiBatchNorm) and not isinstance(module, MinkowskiSyncBatchNorm):
            b = module.bn
            out = cls(b.num_features, b.eps, b.momentum, b.affine, b.track_running_stats, process_group)
            if b.affine:
                with torch.no_grad():
                    out.bn.weight = b.weight
                    out.bn.bias = b.bias
            out.bn.running_mean = b.running_mean
            out.bn.running_var = b.running_var
            out.bn.num_batches_tracked = b.num_batches_tracked
            out.train(module.training)
        for name, child in module.named_children():
            out.add_module(name, cls.convert_sync_batchnorm(child, process_group))
        return out


class InstanceNormFunction(torch.autograd.Function):
    """y = (x - mean[scene]) * rstd[scene] * weight + bias on the engine (lgs_in_forward / lgs_in_backward); keeps x and the
    per-scene (mean, rstd), not y.  `sm`: the origin segment map of x's coordinate map."""

    @staticmethod
    def forward(ctx, x, weight, bias, sm, eps, backend):
        w32, b32 = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        y, stats = backend.instance_norm_forward(sm, x, w32, b32, eps)
        ctx.save_for_backward(x, stats, w32)
        ctx.sm, ctx.backend = sm, backend
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stats, w32 = ctx.saved_tensors
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        dx, dw, db = ctx.backend.instance_norm_backward(ctx.sm, x, dy.contiguous(), w32, stats)
        return dx, dw.view(1, -1), db.view(1, -1), None, None, None


class MinkowskiInstanceNorm(nn.Module):
    """Per-scene normalisation: mean / biased variance over the rows of one batch index, per channel (the heads of
    Res16UNet34Dv2 / Dv3, clip_models.py:416,431; BasicBlockIN[BN]).  HIP tensors run on the engine's per-scene kernels
    (tuning knob INSTANCE_NORM=0: the torch lines below, which CPU tensors always take)."""

    def __init__(self, num_features):
        super().__init__()
        self.num_features = num_features
        self.eps = 1e-6
        self.weight = nn.Parameter(torch.ones(1, num_features))
        self.bias = nn.Parameter(torch.zeros(1, num_features))

    def forward(self, input):
        x = input.F
        backend = get_backend()
        if x.is_cuda and hasattr(backend, "instance_norm_forward") and backend.instance_norm_enabled():
            mgr = input.coordinate_manager
            sm = mgr.segment_map_handle(input.coordinate_map_key, mgr.origin_key())
            w = self.weight if self.weight.dtype == torch.float32 else self.weight.float()
            b = self.bias if self.bias.dtype == torch.float32 else self.bias.float()
            y = InstanceNormFunction.apply(x.contiguous(), w, b, sm, self.eps, backend)
            return input._like(y)
        b = input.C[:, 0].long()
        nb = int(b.max().item()) + 1 if b.numel() else 0
        cnt = torch.zeros(nb, device=x.device, dtype=torch.float32).index_add_(0, b, torch.ones_like(b, dtype=torch.float32))
        xf = x.float()
        mean = torch.zeros(nb, x.shape[1], device=x.device).index_add_(0, b, xf) / cnt[:, None]
        d = xf - mean[b]
        var = torch.zeros(nb, x.shape[1], device=x.device).index_add_(0, b, d * d) / cnt[:, None]
        y = d / torch.sqrt(var[b] + self.eps) * self.weight + self.bias
        return input._like(y.to(x.dtype))


# ------------------------------------------------------------------------------------------ pointwise
class MinkowskiNonlinearityBase(MinkowskiModuleBase):
    MODULE = None

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.module = self.MODULE(*args, **kwargs)

    def forward(self, input):
        return SparseTensor(self.module(input.F), coordinate_map_key=input.coordinate_map_key,
                            coordinate_manager=input.coordinate_manager)

    def __repr__(self):
        return self.__class__.__name__ + "()"


class MinkowskiReLU(MinkowskiNonlinearityBase):
    MODULE = nn.ReLU

    def forward(self, input):
        # in place on the pending result of a norm nobody has read yet: that norm's ReLU epilogue (me/deferred.py); the SAME tensor
        # object comes back -- ME returns a new wrapper of the same (in-place rectified) storage, the two are indistinguishable
        if input._op is not None and self.module.inplace and _deferred.relu_inplace(input):
            return input
        return super().forward(input)


class MinkowskiSigmoid(MinkowskiNonlinearityBase):
    MODULE = nn.Sigmoid


class MinkowskiTanh(MinkowskiNonlinearityBase):
    MODULE = nn.Tanh


class MinkowskiLeakyReLU(MinkowskiNonlinearityBase):
    MODULE = nn.LeakyReLU


class MinkowskiELU(MinkowskiNonlinearityBase):
    MODULE = nn.ELU


class MinkowskiDropout(MinkowskiNonlinearityBase):
    MODULE = nn.Dropout


class MinkowskiLinear(nn.Module):
    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, bias=bias)

    def forward(self, input):
        return input._like(self.linear(input.F))


# ------------------------------------------------------------------------------------------ pooling / broadcast
class PoolingMode(Enum):
    """MinkowskiEngine's pooling modes.  The three GLOBAL_*_POOLING variants of one reduction (DEFAULT / KERNEL /
    PYTORCH_INDEX: implementation choices in ME) all run the same engine kernels here."""
    LOCAL_SUM_POOLING = 0
    LOCAL_AVG_POOLING = 1
    LOCAL_MAX_POOLING = 2
    GLOBAL_SUM_POOLING_DEFAULT = 3
    GLOBAL_AVG_POOLING_DEFAULT = 4
    GLOBAL_MAX_POOLING_DEFAULT = 5
    GLOBAL_SUM_POOLING_KERNEL = 6
    GLOBAL_AVG_POOLING_KERNEL = 7
    GLOBAL_MAX_POOLING_KERNEL = 8
    GLOBAL_SUM_POOLING_PYTORCH_INDEX = 9
    GLOBAL_AVG_POOLING_PYTORCH_INDEX = 10
    GLOBAL_MAX_POOLING_PYTORCH_INDEX = 11


def _pool_op(mode):
    """PoolingMode -> "sum" / "avg" / "max" """
    return mode.name.split("_")[1].lower()


def _need_engine(what):
    backend = get_backend()
    if not hasattr(backend, "pool_reduce"):
        raise RuntimeError("%s needs the HIP engine: backend %r has no pooling kernels (there is no fallback)"
                           % (what, getattr(backend, "name", backend)))
    return backend


_MAX_POOL_LOG2 = 8      # coarsest target the coordinate manager counts at insert time: stride 2^8 relative to the input


def _pow2_window(name, kernel_size, stride, dilation, kernel_generator, dimension):
    """-> the stride s = kernel_size = 2^k of a supported local pooling window; NotImplementedError for anything else"""
    if kernel_generator is None:
        assert dimension is not None and dimension > 0, "dimension must be a positive integer"
        kernel_generator = KernelGenerator(kernel_size=kernel_size, stride=stride, dilation=dilation, dimension=dimension)
    kg = kernel_generator
    ks, st, dil = kg.kernel_size, kg.kernel_stride, kg.kernel_dilation
    k0 = ks[0]
    ok = (kg.dimension == 3 and kg.region_type == RegionType.HYPER_CUBE and all(d == 1 for d in dil)
          and all(k == k0 for k in ks) and all(t == k0 for t in st) and k0 >= 2 and k0 & (k0 - 1) == 0
          and k0 <= (1 << _MAX_POOL_LOG2))
    if not ok:
        raise NotImplementedError(
            "%s(kernel_size=%s, stride=%s, dilation=%s, dimension=%d) is not supported: the engine pools non-overlapping "
            "windows only -- kernel_size == stride == 2^k (2, 4, ..., %d), dilation 1, HYPER_CUBE, D = 3"
            % (name, ks, st, dil, kg.dimension, 1 << _MAX_POOL_LOG2))
    return kg, k0


class _SegReduceFunction(torch.autograd.Function):
    """out[q] = sum / mean / max over the fine rows of coarse row q (lgs_seg_reduce); backward: the segmented broadcast of dy
    (sum: copy, avg: divided by the rows of q) or, for max, dy to the arg-max row of each (q, channel)."""

    @staticmethod
    def forward(ctx, x, sm, op, backend):
        y, amax = backend.pool_reduce(sm, op, x)
        ctx.sm, ctx.op, ctx.backend, ctx.amax = sm, op, backend, amax
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.op == "max":
            dx = ctx.backend.pool_max_backward(ctx.sm, dy, ctx.amax)
        else:
            dx = ctx.backend.pool_broadcast(ctx.sm, "copy" if ctx.op == "sum" else "scale", dy)
        return dx, None, None, None


class _SegCopyFunction(torch.autograd.Function):
    """fine row r <- coarse row q of r (lgs_seg_broadcast "copy"): the unpooling of a kernel_size == stride window, where
    each output row has exactly one contributor; backward: the segmented sum"""

    @staticmethod
    def forward(ctx, g, sm, backend):
        ctx.sm, ctx.backend = sm, backend
        return backend.pool_broadcast(sm, "copy", g)

    @staticmethod
    def backward(ctx, dy):
        return ctx.backend.pool_reduce(ctx.sm, "sum", dy)[0], None, None


class _BroadcastFunction(torch.autograd.Function):
    """out[r] = x[r] + g[b(r)] ("add"), x[r] * g[b(r)] ("mul"), [x[r], g[b(r)]] ("cat"), g[b(r)] ("copy"); g is a global-pooled
    tensor (one row per batch index).  d g = per-batch segmented sum of dy (of dy * x for "mul", of dy's g columns for "cat")."""

    @staticmethod
    def forward(ctx, x, g, sm, op, backend):
        ctx.sm, ctx.op, ctx.backend = sm, op, backend
        if op == "mul":
            ctx.save_for_backward(x, g)
        if op in ("add", "mul"):
            return backend.pool_broadcast(sm, op, g, x)
        if op == "copy":
            return backend.pool_broadcast(sm, "copy", g)
        ctx.cx = x.shape[1]
        out = torch.empty((sm.n_fine, x.shape[1] + g.shape[1]), dtype=x.dtype, device=x.device)
        backend.pool_broadcast(sm, "copy_x", None, x, out=out, col=0)
        backend.pool_broadcast(sm, "copy", g, out=out, col=x.shape[1])
        return out

    @staticmethod
    def backward(ctx, dy):
        sm, op, be = ctx.sm, ctx.op, ctx.backend
        dx = dg = None
        if op == "add":
            dx = dy if ctx.needs_input_grad[0] else None
            dg = be.pool_reduce(sm, "sum", dy)[0] if ctx.needs_input_grad[1] else None
        elif op == "mul":
            x, g = ctx.saved_tensors
            dy = dy.contiguous()
            dx = be.pool_broadcast(sm, "mul", g, dy) if ctx.needs_input_grad[0] else None
            dg = be.pool_reduce(sm, "prod", dy, x.contiguous())[0] if ctx.needs_input_grad[1] else None
        elif op == "copy":
            dg = be.pool_reduce(sm, "sum", dy)[0] if ctx.needs_input_grad[1] else None
        else:
            dx = dy[:, :ctx.cx] if ctx.needs_input_grad[0] else None
            dg = be.pool_reduce(sm, "sum", dy[:, ctx.cx:])[0] if ctx.needs_input_grad[1] else None
        return dx, dg, None, None, None


class MinkowskiPoolingBase(MinkowskiModuleBase):
    """Local pooling over non-overlapping 2^k windows: the output lives on the map stride 2 makes k times, the map a
    (kernel 2, stride 2) convolution would produce, so the two outputs share their coordinate_map_key."""
    MODE = None

    def __init__(self, kernel_size=-1, stride=1, dilation=1, kernel_generator=None, dimension=None):
        super().__init__()
        self.kernel_generator, s = _pow2_window(self.__class__.__name__, kernel_size, stride, dilation, kernel_generator, dimension)
        self.kernel_size = self.kernel_generator.kernel_size
        self.stride = self.kernel_generator.kernel_stride
        self.dilation = self.kernel_generator.kernel_dilation
        self.dimension = self.kernel_generator.dimension
        self.pooling_mode = self.MODE
        self._s = s

    def forward(self, input, coordinates=None):
        assert isinstance(input, SparseTensor)
        assert coordinates is None, "explicit output coordinates are not supported"
        backend = _need_engine(self.__class__.__name__)
        mgr = input.coordinate_manager
        out_key = mgr.coarser_key(input.coordinate_map_key, self._s)
        sm = mgr.segment_map_handle(input.coordinate_map_key, out_key)
        y = _SegReduceFunction.apply(input.F, sm, _pool_op(self.MODE), backend)
        return SparseTensor(y, coordinate_map_key=out_key, coordinate_manager=mgr)

    def __repr__(self):
        return "%s(kernel_size=%s, stride=%s, dilation=%s)" % (self.__class__.__name__, self.kernel_size, self.stride, self.dilation)


class MinkowskiSumPooling(MinkowskiPoolingBase):
    MODE = PoolingMode.LOCAL_SUM_POOLING


class MinkowskiAvgPooling(MinkowskiPoolingBase):
    """average over the input rows PRESENT in the window (ME's rule), not over the kernel volume"""
    MODE = PoolingMode.LOCAL_AVG_POOLING


class MinkowskiMaxPooling(MinkowskiPoolingBase):
    """per-channel maximum; its gradient goes to one input row per (output row, channel): on ties the smallest row index"""
    MODE = PoolingMode.LOCAL_MAX_POOLING


class MinkowskiPoolingTranspose(MinkowskiModuleBase):
    """Unpooling of a kernel_size == stride == 2^k window onto the cached map 2^k times finer (the one the matching pooling or
    strided convolution came from).  Each output row has exactly one contributing input row, so ME's "sum of contributors /
    their count" is a copy; the backward pass is the segmented sum."""

    def __init__(self, kernel_size=-1, stride=1, dilation=1, kernel_generator=None, expand_coordinates=False, dimension=None):
        super().__init__()
        if expand_coordinates:
            raise NotImplementedError("%s(expand_coordinates=True) is not supported" % self.__class__.__name__)
        self.kernel_generator, s = _pow2_window(self.__class__.__name__, kernel_size, stride, dilation, kernel_generator, dimension)
        self.kernel_size = self.kernel_generator.kernel_size
        self.stride = self.kernel_generator.kernel_stride
        self.dilation = self.kernel_generator.kernel_dilation
        self.dimension = self.kernel_generator.dimension
        self._s = s

    def forward(self, input, coordinates=None):
        assert isinstance(input, SparseTensor)
        assert coordinates is None, "explicit output coordinates are not supported"
        backend = _need_engine(self.__class__.__name__)
        mgr = input.coordinate_manager
        out_key = mgr.finer_key_by(input.coordinate_map_key, self._s)
        sm = mgr.segment_map_handle(out_key, input.coordinate_map_key)
        y = _SegCopyFunction.apply(input.F, sm, backend)
        return SparseTensor(y, coordinate_map_key=out_key, coordinate_manager=mgr)

    def __repr__(self):
        return "%s(kernel_size=%s, stride=%s, dilation=%s)" % (self.__class__.__name__, self.kernel_size, self.stride, self.dilation)


class MinkowskiAvgUnpooling(MinkowskiPoolingTranspose):
    """with kernel_size == stride every output row has one contributor: the same copy as MinkowskiPoolingTranspose"""


class MinkowskiGlobalPooling(MinkowskiModuleBase):
    """One output row per batch index present in the input, in ascending batch order, on the manager's origin map
    (`.C` = [b, 0, 0, 0]).  Default: average, as in ME."""
    KIND = None

    def __init__(self, mode=PoolingMode.GLOBAL_AVG_POOLING_DEFAULT):
        super().__init__()
        if not isinstance(mode, PoolingMode) or not mode.name.startswith("GLOBAL_"):
            raise ValueError("%s: mode must be a global PoolingMode, got %r" % (self.__class__.__name__, mode))
        if self.KIND is not None and _pool_op(mode) != self.KIND:
            raise ValueError("%s: mode %s is not a global %s pooling mode" % (self.__class__.__name__, mode.name, self.KIND))
        self.pooling_mode = mode

    def forward(self, input, coordinates=None):
        assert isinstance(input, SparseTensor)
        assert coordinates is None, "explicit output coordinates are not supported"
        backend = _need_engine(self.__class__.__name__)
        mgr = input.coordinate_manager
        out_key = mgr.origin_key()
        sm = mgr.segment_map_handle(input.coordinate_map_key, out_key)
        y = _SegReduceFunction.apply(input.F, sm, _pool_op(self.pooling_mode), backend)
        return SparseTensor(y, coordinate_map_key=out_key, coordinate_manager=mgr)

    def __repr__(self):
        return "%s(mode=%s)" % (self.__class__.__name__, self.pooling_mode.name)


class MinkowskiGlobalSumPooling(MinkowskiGlobalPooling):
    KIND = "sum"

    def __init__(self, mode=PoolingMode.GLOBAL_SUM_POOLING_DEFAULT):
        super().__init__(mode)


class MinkowskiGlobalAvgPooling(MinkowskiGlobalPooling):
    KIND = "avg"

    def __init__(self, mode=PoolingMode.GLOBAL_AVG_POOLING_DEFAULT):
        super().__init__(mode)


class MinkowskiGlobalMaxPooling(MinkowskiGlobalPooling):
    KIND = "max"

    def __init__(self, mode=PoolingMode.GLOBAL_MAX_POOLING_DEFAULT):
        super().__init__(mode)


class MinkowskiBroadcastBase(MinkowskiModuleBase):
    """`module(x, g)` (ME 0.5): x a SparseTensor, g a global-pooled SparseTensor of the same manager; the output lives on x's
    map and row i combines x[i] with g[batch(i)]."""
    OP = None

    def __init__(self):
        super().__init__()

    def forward(self, input, input_glob):
        assert isinstance(input, SparseTensor) and isinstance(input_glob, SparseTensor)
        backend = _need_engine(self.__class__.__name__)
        mgr = input.coordinate_manager
        if input_glob.coordinate_manager is not mgr or input_glob.coordinate_map_key != mgr.origin_key():
            raise ValueError("%s: the second input must be a global-pooled tensor of the first input's coordinate manager"
                             % self.__class__.__name__)
        sm = mgr.segment_map_handle(input.coordinate_map_key, input_glob.coordinate_map_key)
        g = input_glob.F
        if self.OP == "copy":
            y = _BroadcastFunction.apply(None, g, sm, "copy", backend)
        else:
            x = input.F
            if x.dtype != g.dtype:
                raise ValueError("%s: both inputs must share one dtype (%s vs %s)" % (self.__class__.__name__, x.dtype, g.dtype))
            if self.OP != "cat" and x.shape[1] != g.shape[1]:
                raise ValueError("%s: channel counts differ (%d vs %d)" % (self.__class__.__name__, x.shape[1], g.shape[1]))
            y = _BroadcastFunction.apply(x, g, sm, self.OP, backend)
        return SparseTensor(y, coordinate_map_key=input.coordinate_map_key, coordinate_manager=mgr)

    def __repr__(self):
        return self.__class__.__name__ + "()"


class MinkowskiBroadcast(MinkowskiBroadcastBase):
    """g[batch(i)] on x's map (x contributes its coordinates only)"""
    OP = "copy"


class MinkowskiBroadcastAddition(MinkowskiBroadcastBase):
    OP = "add"


class MinkowskiBroadcastMultiplication(MinkowskiBroadcastBase):
    OP = "mul"


class MinkowskiBroadcastConcatenation(MinkowskiBroadcastBase):
    """[x[i], g[batch(i)]] (x's channels first)"""
    OP = "cat"
