"""Host-side decisions every engine wrapper shares, one answer each:
  rows_in_place    can this [n, c] operand be read / written in place as a column slice of a wider buffer?
  relu_mode_of     which ReLU mask a norm's backward uses
  GradSink         where a parameter gradient goes: the bucket slot or fp32 scratch (AffineSink / WeightSink build one)
  wgrad_placement  which stream a weight gradient runs on (+ the side-stream book-keeping BucketedDDP reads)
  memo             the one cache of engine size / plan queries
Imports torch, engine and tuning only: backend_hip, modules, block and ddp all import it.  How a caller hands addresses, streams and
scratch to the C-ABI is the call layer's business: ../hipcall.py, under the same import rule."""
import torch

from .. import engine
from .. import tuning as _tuning

_WIDE_WGRAD_INLINE = _tuning.host("WIDE_WGRAD_INLINE") != 0
_DBG_WGRAD = _tuning.host("DBG_WGRAD")   # "", "skip", "inline": step-time attribution experiments only


# ------------------------------------------------------------------------------------------ operands read in place
def row_stride(t, c):
    """row stride (elements) if `t` [n, c] is a column slice of a wider row-major tensor the kernels can address in place
    (16-byte aligned rows), else 0"""
    if t.dim() == 2 and t.shape[1] == c and t.stride(1) == 1 and t.stride(0) > c:
        if (t.stride(0) * t.element_size()) % 16 == 0 and t.data_ptr() % 16 == 0:
            return t.stride(0)
    return 0


def rows_in_place(t, c):
    """-> (tensor, row stride for the engine) of a [n, c] operand: itself and its stride when row_stride allows, else a contiguous
    copy and 0 (the engine reads 0 as c).  None stays None."""
    if t is None:
        return None, 0
    ld = row_stride(t, c)
    return (t, ld) if ld else (t.contiguous(), 0)


def relu_mode_of(relu, has_residual):
    """ReLU mask of a norm's backward: 0 none; 1 from the saved output (a residual was added before the ReLU); 2 recomputed from x
    (the output is not kept alive)"""
    return 0 if not relu else (1 if has_residual else 2)


# ------------------------------------------------------------------------------------------ parameter gradients
def grad_slot_view(param):
    """Fresh view of the parameter's slot in a flat gradient bucket (languagegroundedsemseg_amd.ddp.BucketedDDP), or
    None.  Returning such a view from backward() lets autograd adopt it as `.grad` without an accumulation kernel:
    the engine has already written the gradient where the all-reduce and the optimiser will read it."""
    slot = getattr(param, "_lgs_grad_slot", None)
    if slot is None or param.grad is not None:
        return None
    flat, off, shape = slot
    n = 1
    for d in shape:
        n *= d
    return flat[off:off + n].view(shape)


class GradSink:
    """The buffers the engine writes the gradients of `params` into: every parameter's bucket-slot view (`adopted`: autograd
    takes the views as `.grad`), or -- when any of them has none (no bucket, `.grad` already set, not a Parameter: None) --
    fp32 scratch of `shape` for all of them, never a mixture.  shape=None: no scratch is made (`bufs` is None), for callers whose
    engine call allocates its own result."""
    __slots__ = ("bufs", "adopted")

    def __init__(self, params, shape, device):
        views = []
        for p in params:                      # (plain loop: this runs ~100 times per backward of a host-bound step)
            v = grad_slot_view(p) if p is not None else None
            if v is None:
                break
            views.append(v)
        self.adopted = len(views) == len(params)
        if self.adopted:
            self.bufs = tuple(views)
        elif shape is None:
            self.bufs = None
        elif len(params) == 1:
            self.bufs = (torch.empty(shape, dtype=torch.float32, device=device),)
        else:
            self.bufs = torch.empty((len(params),) + tuple(shape), dtype=torch.float32, device=device).unbind(0)

    def returned(self, dtype, need=True):
        """what backward() returns for these parameters: the adopted views, else the scratch cast to the parameter dtype, or
        None each when the caller does not `need` them"""
        if self.adopted:
            return self.bufs
        if not need:
            return (None,) * len(self.bufs)
        return tuple(b.to(dtype) for b in self.bufs)


def AffineSink(gparam, bparam, c, device):
    """d gamma / d beta [c] of one norm -> GradSink; bufs = (dgamma, dbeta)"""
    return GradSink((gparam, bparam), (c,), device)


def WeightSink(kparam, shape=None, device=None):
    """the weight gradient of one convolution -> GradSink; bufs = (gw,)"""
    return GradSink((kparam,), shape, device)


# ------------------------------------------------------------------------------------------ weight-gradient placement
def wgrad_placement(slot, cin, cout, rows, inline_wgrad):
    """Where modules.conv_weight_grad runs one weight gradient.  slot: it goes into a bucket slot on a device with a side stream.
      "plain"   no slot: the engine's own fp32 result on the compute stream, cast by the caller
      "skip"    DBG_WGRAD=skip (profiling): no weight gradient at all
      "inline"  into the slot on the compute stream: DBG_WGRAD=inline, a small (host-bound) batch (`inline_wgrad`, set by the manager
                below WGRAD_INLINE_BELOW voxels: no fork / join events, no second stream to feed), or a wide layer -- >= 256 x 256
                channels on >= 65536 rows: the weight gradient (k_wgrad_wide / wide k_wgrad_ps) and the dgrad beside it
                (k_conv_wide) are MFMA-bound kernels that own their CUs, concurrently they halve each other (CLIP step: dgrad 17.5 ms
                in-step vs 9.2 alone, weight gradient 15.9 vs 7.7), so there is nothing to overlap (WIDE_WGRAD_INLINE=0 turns the
                rule off; the 256-channel layers of the coarse levels are latency-bound launches that DO overlap)
      "side"    into the slot on the side stream, off the critical path dgrad -> BN -> dgrad
    HipBackend.block_backward (one engine call for the three weight gradients of a block) decides from the same pieces but not the
    same rule: there one parameter without a slot pulls all three gradients onto the compute stream, any DBG_WGRAD value other than
    "" means inline (it has no "skip"), and it has no wide rule."""
    if not slot:
        return "plain"
    if _DBG_WGRAD == "skip":
        return "skip"
    wide = _WIDE_WGRAD_INLINE and cin >= 256 and cout >= 256 and rows >= 65536
    if _DBG_WGRAD == "inline" or wide or inline_wgrad:
        return "inline"
    return "side"


_WGRAD_SEQ = [0]     # issue order of the side-stream weight gradients (the stream runs them in this order)


def param_event(param):
    """the reusable event recorded behind a kernel parameter's side-stream weight gradient: BucketedDDP waits for exactly the
    weight gradients of the bucket it is about to reduce (ddp._wait_bucket_wgrads), not for the whole side stream"""
    ev = getattr(param, "_lgs_wgrad_event", None)
    if ev is None:
        ev = param._lgs_wgrad_event = torch.cuda.Event()
    return ev


def note_side_wgrad(kparam):
    """book-keeping of one weight gradient issued on the side stream (by conv_weight_grad, or by lgs_block_backward): its place in
    the stream's order and the step it belongs to -- BucketedDDP picks the newest event of a bucket from these"""
    _WGRAD_SEQ[0] += 1
    kparam._lgs_wgrad_seq = _WGRAD_SEQ[0]
    owner = getattr(kparam, "_lgs_ddp", None)
    kparam._lgs_wgrad_step = owner._step if owner is not None else -1


def side_wgrads_issued(side, kparams, operands):
    """after weight gradients of `kparams` (in issue order) were enqueued on `side`: note them, and keep the memory of the
    operands they read from being reused before that stream is done with it"""
    for p in kparams:
        note_side_wgrad(p)
    for t in operands:
        t.record_stream(side)


# ------------------------------------------------------------------------------------------ engine queries
def memo(cache, key, ask, *args):
    """cache[key] or ask(*args).  Sizes and plans the engine answers depend on tuning knobs, so every key carries
    engine.TUNING_EPOCH (a size cached across engine.tuning(...) once let a kernel write its padded fp32 input past the
    workspace); a cache that outgrows 4096 entries starts over."""
    key += (engine.TUNING_EPOCH,)
    try:
        return cache[key]
    except KeyError:
        if len(cache) > 4096:
            cache.clear()
        v = cache[key] = ask(*args)
        return v
