"""EmbeddingVariable -- the GPU-resident counterpart of DeepRec's
python/ops/kv_variable_ops.py:44-765 (class EmbeddingVariable) and
python/ops/variables.py:238-330 (EmbeddingVariableOption / CounterFilter /
CBFFilter).  Storage and the insert-on-miss lookup run in HIP kernels through
the C ABI (dr_ev_*); this module only holds the handle and the Python-level
argument semantics.
"""
import ctypes as C
import atexit
import collections
import threading

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_handle, workspace


# ---------------------------------------------------------------------------
# Options (variables.py:238-330)
# ---------------------------------------------------------------------------
class CounterFilter(object):
    def __init__(self, filter_freq=0):
        self.filter_freq = filter_freq


class CBFFilter(object):
    """Counting Bloom filter admission (embedding_filter.h:27-286)."""

    def __init__(self, filter_freq=0, max_element_size=0, false_positive_probability=-1.0,
                 counter_type=torch.int64):
        self.filter_freq = filter_freq
        self.max_element_size = max_element_size
        self.false_positive_probability = false_positive_probability
        bits = {torch.uint8: 8, torch.int8: 8, torch.int16: 16, torch.int32: 32,
                torch.int64: 64}
        self.counter_bits = bits.get(counter_type, 64) if not isinstance(counter_type, int) \
            else counter_type


class GlobalStepEvict(object):
    def __init__(self, steps_to_live=None):
        self.steps_to_live = steps_to_live


_EVICT_POLICIES = {"lru": 0, "lfu": 1}      # DR_EVICT_LRU / DR_EVICT_LFU


class KeyBudgetEvict(object):
    """A key budget for the table in HBM (build-defined):
    at a save the key space keeps at most `max_keys` keys and the coldest go,
    by version ("lru", needs steps_to_live != 0) or by freq ("lfu", needs a
    CounterFilter).  max_keys 0 is off.  `steps_to_live` is GlobalStepEvict's,
    so the age rule and the budget can be set together."""

    def __init__(self, max_keys, policy="lru", steps_to_live=None):
        if policy not in _EVICT_POLICIES:
            raise ValueError("KeyBudgetEvict: policy is 'lru' or 'lfu', not %r" % (policy,))
        self.max_keys = int(max_keys)
        self.policy = policy
        self.steps_to_live = steps_to_live


class StorageType(object):
    """Where an EmbeddingVariable keeps its keys (config.proto StorageType;
    the tiers below DRAM are not built)."""
    HBM = "HBM"
    HBM_DRAM = "HBM_DRAM"


class StorageOption(object):
    """StorageType.HBM_DRAM (build-defined): the keys a
    KeyBudgetEvict budget pushes out of HBM are demoted to host DRAM with
    their rows, optimizer slots, version, freq and admission state, and a
    lookup that names one promotes it back first -- the table trains as an
    unbudgeted one in HBM would.  incremental=True (HBM_DRAM only; DESIGN
    section 17) also lets the key space track updates and removals and write
    and apply incremental checkpoints: the update bit and the removal log
    follow a key across the tiers.  Without it those calls are refused."""

    def __init__(self, storage_type=StorageType.HBM, incremental=False):
        if storage_type not in (StorageType.HBM, StorageType.HBM_DRAM):
            raise ValueError("StorageOption: storage_type is StorageType.HBM or "
                             "StorageType.HBM_DRAM, not %r" % (storage_type,))
        if incremental and storage_type != StorageType.HBM_DRAM:
            raise ValueError("StorageOption: incremental=True is the opt-in of a "
                             "StorageType.HBM_DRAM key space (an HBM one needs none)")
        self.storage_type = storage_type
        self.incremental = bool(incremental)


MAX_INIT_TABLE_ROWS = 1 << 20     # DR_MAX_INIT_TABLE_ROWS


class InitializerOption(object):
    """variables.py InitializerOption: the initializer is
    run once, for a [default_value_dim, dim] table, and a new key k starts from
    table row k % default_value_dim (EmbeddingVar::GetDefaultValue) -- a floor
    mod, so the initial row is a function of the key alone.  A key the filter
    has not admitted (and a read-only miss) reads a row of
    default_value_no_permission.  initializer None: the EV's own initializer=
    argument; a constant is broadcast."""

    def __init__(self, initializer=None, default_value_dim=4096, default_value_no_permission=0.0):
        k = int(default_value_dim)
        if k < 1 or k > MAX_INIT_TABLE_ROWS:
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "InitializerOption: default_value_dim must be in "
                "[1, %d], not %d" % (MAX_INIT_TABLE_ROWS, k))
        self.initializer = initializer
        self.default_value_dim = k
        self.default_value_no_permission = float(default_value_no_permission)


class EmbeddingVariableOption(object):
    # The constructor's parameter list is pinned (tests/test_host_tier_abi.py), so
    # the InitializerOption is an attribute: set it, or chain with_init_option().
    init_option = None

    def __init__(self, ht_type="", ht_partition_num=1000, evict_option=None, filter_option=None,
                 storage_option=None):
        self.ht_type = ht_type
        self.ht_partition_num = ht_partition_num
        self.evict_option = evict_option
        self.filter_option = filter_option
        self.storage_option = storage_option

    def with_init_option(self, init_option):
        """Set the InitializerOption and return self:
        EmbeddingVariableOption(...).with_init_option(InitializerOption(...))."""
        self.init_option = init_option
        return self


def _default_row(initializer, dim, device, dtype=torch.float32):
    """EV default_value_ (InitializeKvVariableOp input 2, a [dim] tensor)."""
    if initializer is None:
        initializer = 0.0
    if callable(initializer):
        v = initializer((dim,))
        v = torch.as_tensor(v, dtype=dtype).reshape(dim)
    else:
        v = torch.full((dim,), float(initializer), dtype=dtype)
    return v.cpu().contiguous()


def _init_table_host(init_option, initializer, dim, dtype=torch.float32, name=""):
    """The [default_value_dim, dim] host table of an InitializerOption: its
    initializer (or else the EV's) called once with that shape; a constant is
    broadcast."""
    k = int(init_option.default_value_dim)
    if k < 1 or k > MAX_INIT_TABLE_ROWS:       # (the attribute may have been reassigned)
        raise _lib.InvalidArgumentError(
            _lib.INVALID_ARGUMENT, "InitializerOption: default_value_dim must be in [1, %d], "
            "not %d (%s)" % (MAX_INIT_TABLE_ROWS, k, name))
    ini = init_option.initializer if init_option.initializer is not None else initializer
    if ini is None:
        ini = 0.0
    if callable(ini):
        v = torch.as_tensor(ini((k, dim)), dtype=dtype)
        if tuple(v.shape) != (k, dim):
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "InitializerOption: the initializer returned shape %s "
                "for (%d, %d) (%s)" % (tuple(v.shape), k, dim, name))
    else:
        v = torch.full((k, dim), float(ini), dtype=dtype)
    return v.cpu().contiguous()


# Handles whose last Python reference died.  Releasing one frees device
# memory (hipFree) and synchronises, which breaks a hipGraph capture in
# torch's default global mode if ANY stream of the process is capturing --
# and __del__ runs on whatever thread triggers the collection, whose own
# current stream says nothing about another thread's capture.  So __del__
# never releases: it queues the handle, and the queue is flushed at points
# where the library itself runs uncaptured host work (EV creation, the end
# of an optimizer's apply_gradients) and by flush_releases() -- and only when
# no capture is open anywhere in the process: torch.cuda.CUDAGraph's
# capture_begin / capture_end are counted process-wide (_CAPTURES), on every
# thread.  At interpreter exit the queue is dropped (the process's device
# memory goes with it).
# __del__ appends without the lock (deque.append is atomic): a collection
# that runs inside the locked flush below, on the same thread, must not block
# on the lock that thread holds.  The lock is reentrant for the same reason.
_DEFERRED = collections.deque()
_DEFERRED_LOCK = threading.RLock()
_CAPTURES = [0]     # torch graph captures open in this process (any thread)


def _install_capture_counter():
    G = getattr(torch.cuda, "CUDAGraph", None)
    if G is None or getattr(G, "_dr_counted", False):
        return
    begin, end = G.capture_begin, G.capture_end

    def capture_begin(self, *a, **k):
        with _DEFERRED_LOCK:
            _CAPTURES[0] += 1
        try:
            return begin(self, *a, **k)
        except BaseException:
            with _DEFERRED_LOCK:
                _CAPTURES[0] -= 1
            raise

    def capture_end(self, *a, **k):
        try:
            return end(self, *a, **k)
        finally:
            with _DEFERRED_LOCK:
                _CAPTURES[0] -= 1

    G.capture_begin, G.capture_end, G._dr_counted = capture_begin, capture_end, True


_install_capture_counter()


def _capturing():
    """A capture is open on this thread's stream or on any thread (torch)."""
    if _CAPTURES[0] > 0:
        return True
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _flush_deferred_releases():
    if not _DEFERRED:
        return
    # the lock is held across the frees: a capture_begin on another thread
    # waits for them instead of starting in between
    with _DEFERRED_LOCK:
        if _CAPTURES[0] > 0:
            return
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return
        while True:
            try:
                h = _DEFERRED.popleft()
            except IndexError:
                break
            if isinstance(h, tuple):      # (destroy entry name, handle): engines
                getattr(lib(), h[0])(h[1])
            else:
                lib().dr_ev_release(h)


def flush_releases():
    """Release the device memory of every EmbeddingVariable that has been
    garbage-collected (call outside any hipGraph capture)."""
    if _capturing():
        raise RuntimeError("flush_releases() inside a stream capture")
    _flush_deferred_releases()


def _release_handle(h):
    _DEFERRED.append(h)   # lock-free: may run from GC inside the flush


def _release_engine(destroy, h):
    """Queue an engine handle (e.g. dr_sharded_destroy, which synchronises the
    device) on the same capture-safe deferred path as EV handles."""
    _DEFERRED.append((destroy, h))


atexit.register(lambda: _DEFERRED.clear())   # dropped: the process's device memory goes too


# ---------------------------------------------------------------------------
# Read-only lookups (EmbeddingVar::Lookup, the reference's inference mode)
# ---------------------------------------------------------------------------
_READ_ONLY = threading.local()


def read_only_active():
    return getattr(_READ_ONLY, "depth", 0) > 0


def read_only_serves_tier():
    """Inside read_only_lookups(serve_tier=True), or a block nested in one."""
    return read_only_active() and getattr(_READ_ONLY, "serve_tier", False)


class read_only_lookups(object):
    """Context manager (re-entrant, per thread): inside it embedding_lookup,
    embedding_lookup_sparse[_multi] and safe_embedding_lookup_sparse read
    EmbeddingVariables without changing them -- evaluation and serving.  A
    present, admitted id gives its row, any other the EV's default row; no
    key is created, no sighting counted, no table grown; results carry no
    grad_fn and nothing is queued in pending_grads.  Dense tables and
    tensors behave as outside it.  The sharded lookup engines (sharded.py)
    follow it too: their owners serve without inserting, and an id its
    owner does not serve reads that OWNER's default row.

    serve_tier=True (inherited by the blocks nested in it): the pooled
    lookups of an HBM_DRAM EmbeddingVariable serve the ids its host-DRAM tier
    holds from the tier, in place -- neither tier changes -- instead of
    refusing the batch."""

    def __init__(self, *, serve_tier=False):
        self._serve_tier = bool(serve_tier)
        self._outer = []

    def __enter__(self):
        _READ_ONLY.depth = getattr(_READ_ONLY, "depth", 0) + 1
        outer = getattr(_READ_ONLY, "serve_tier", False)
        self._outer.append(outer)
        _READ_ONLY.serve_tier = outer or self._serve_tier
        return self

    def __exit__(self, *exc):
        _READ_ONLY.depth -= 1
        _READ_ONLY.serve_tier = self._outer.pop()
        return False


_KEY_DTYPES = (torch.int64, torch.int32)
# bfloat16: a build-defined bf16 EV (BASELINE configs[4]; the reference
# registers float and double): bf16 value rows, fp32 optimizer slots
_VALUE_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


class IndexedSlices(object):
    """values [N, D] for rows `indices` [N] (tf.IndexedSlices).

    A lookup backward may hand the values over BY ADDRESS instead
    (dr_pool_grad_rows_grouped): grad_ptr [N] int64 holds the address of
    each row (bit 0: use as 0.0f + g) and `keep` the buffers they point into.
    The EV optimizers read such rows in place (dr_ev_apply_grouped_ptr);
    `values` materialises them on first access (dr_rows_from_ptr)."""

    def __init__(self, values, indices, num_valid=None, unique=False, grad_ptr=None, dim=None,
                 keep=(), rows=None):
        self._values = values
        self.indices = indices
        # rows [N] int64: the EV row each index was resolved to by the forward
        # (a row-grouped backward); lets SGD skip the key-table probe
        self.rows = rows
        self.num_valid = num_valid  # optional device int64[1] (<= N)
        self.unique = unique        # indices known distinct (a lookup's backward)
        self.grad_ptr = grad_ptr
        self.dim = dim
        self._keep = keep

    @property
    def values(self):
        if self._values is None and self.grad_ptr is not None:
            n = self.grad_ptr.numel()
            out = torch.empty((n, self.dim), dtype=torch.float32, device=self.grad_ptr.device)
            _lib.check(_lib.lib().dr_rows_from_ptr(
                _lib.ptr(self.grad_ptr), n, _lib.ptr(self.num_valid), self.dim, _lib.ptr(out),
                _lib.stream_handle(self.grad_ptr.device)))
            self._values = out
        return self._values

    @values.setter
    def values(self, v):
        self._values = v
        self.grad_ptr = None
        self._keep = ()


class PendingRowSlices(IndexedSlices):
    """Table t's gradient of a row-grouped lookup backward, not yet formed.

    An SGD apply_gradients over every variable of the group runs the
    backward fused with the update (dr_ev_pool_grad_rows_apply_sgd: the same
    run sums and v -= lr * g roundings, no IndexedSlices in between).  Any
    other use -- indices, values, rows, num_valid, grad_ptr -- first forms the
    IndexedSlices exactly as the eager backward (dr_pool_grad_rows_grouped_ex)
    would have, and the object is an ordinary IndexedSlices from then on."""

    _LAZY = ("indices", "rows", "num_valid", "grad_ptr", "_values", "_keep")

    def __init__(self, pending, t, dim):
        self._pending = pending
        self._t = t
        self.unique = True
        self.dim = dim

    def __getattr__(self, name):
        # only reached for attributes not yet in __dict__
        if name in PendingRowSlices._LAZY:
            real = self._pending.materialize()[self._t]
            for k in PendingRowSlices._LAZY:
                self.__dict__.setdefault(k, getattr(real, k))
            return self.__dict__[name]
        raise AttributeError(name)

    def fusable(self):
        return "indices" not in self.__dict__ and self._pending.fusable()

    @property
    def values(self):
        return IndexedSlices.values.fget(self)

    @values.setter
    def values(self, v):
        self.__getattr__("indices")   # formed first: the indices stay valid
        IndexedSlices.values.fset(self, v)


class EmbeddingVariable(object):
    """Hash-keyed embedding table resident in HBM.

    initializer: float constant, or callable(shape) -> tensor (e.g.
    lambda s: torch.randn(s) * 0.01).  As in the reference, a callable
    initializer draws a fresh [N, D] default block per sparse_read call
    (kv_variable_ops.py:651-654); a constant uses the EV's own default row.
    With EmbeddingVariableOption().with_init_option(InitializerOption(...)) the
    initializer is called once instead, for the EV's init table on the device:
    a new key k starts from init_table[k % default_value_dim] on every path.
    """

    def __init__(self, name, embedding_dim, initializer=None, steps_to_live=0, ev_option=None,
                 capacity=1 << 16, device=None, _primary=None, _slot_index=0,
                 l2_weight_threshold=-1.0, key_dtype=torch.int64, value_dtype=torch.float32):
        _lib.require_gpu()
        if key_dtype not in _KEY_DTYPES or value_dtype not in _VALUE_DTYPES:
            raise TypeError("EmbeddingVariable keys are int32 / int64 and values float32 / "
                            "float64 (the reference's KvResourceGather registrations) or "
                            "bfloat16 (bf16 EV)")
        self.name = name
        self.dim = int(embedding_dim)
        self.key_dtype = key_dtype
        if _primary is None:
            self.value_dtype = value_dtype
        else:
            # optimizer slots of a bf16 EV keep fp32 state
            pv = _primary.value_dtype
            self.value_dtype = torch.float32 if pv == torch.bfloat16 else pv
        if self.value_dtype == torch.bfloat16 and self.dim % 2:
            raise _lib.DeepRecError(_lib.INVALID_ARGUMENT, "bf16 EVs need an even dim")
        self.device = torch.device(device) if device is not None else \
            torch.device("cuda", torch.cuda.current_device())
        self.initializer = initializer
        self._primary = _primary
        self._slot_index = _slot_index
        self._lock = threading.Lock()
        self._tracking = False    # update tracking of the key space (held by the primary)
        self._tracking_by_row = False   # ... marked by row in apply_gradients
        self.pending_grads = []
        opt = ev_option or EmbeddingVariableOption()
        f = opt.filter_option
        self.filter_freq = int(getattr(f, "filter_freq", 0) or 0)
        if opt.evict_option is not None and opt.evict_option.steps_to_live:
            steps_to_live = opt.evict_option.steps_to_live
        self.steps_to_live = int(steps_to_live or 0)
        # key budget applied by checkpoint.save / save_incremental (KeyBudgetEvict); 0 = off
        self.max_keys = int(getattr(opt.evict_option, "max_keys", 0) or 0)
        self.policy = getattr(opt.evict_option, "policy", "lru")
        # EmbeddingConfig::l2_weight_threshold (embedding_config.h:17,28): -1 = off
        self.l2_weight_threshold = float(l2_weight_threshold)
        # host-DRAM tier of the key space (held by the primary): the store's
        # handle, the columns it was made for and a host mirror of its size,
        # so that an empty tier costs the lookups nothing
        so = opt.storage_option
        self._tiered = _primary is None and so is not None and \
            so.storage_type == StorageType.HBM_DRAM
        self._tier = None
        self._tier_ncols = 0
        self._tier_n = 0
        # StorageOption(..., incremental=True): update bits and the removal log
        # follow the keys across the tiers
        self._tier_incremental = self._tiered and bool(getattr(so, "incremental", False))
        if self._tiered:
            why = None
            if not self.max_keys:
                why = "a KeyBudgetEvict with max_keys > 0 (the HBM budget)"
            elif isinstance(f, CBFFilter) or getattr(f, "max_element_size", 0):
                why = "no Bloom filter (its counters do not travel with a key)"
            elif key_dtype != torch.int64:
                why = "int64 keys"
            elif self.l2_weight_threshold != -1.0:
                why = "l2_weight_threshold == -1 (the L2 rule would need the demoted rows in HBM)"
            if why:
                raise _lib.InvalidArgumentError(
                    _lib.INVALID_ARGUMENT, "StorageType.HBM_DRAM needs %s (%s)" % (why, name))
        _flush_deferred_releases()
        bf16 = self.value_dtype == torch.bfloat16
        # the C ABI takes the default row in fp32 (a bf16 EV rounds it to
        # nearest even, as the .to(torch.bfloat16) below does)
        host_dtype = torch.float32 if bf16 else self.value_dtype
        # InitializerOption (primary EVs; slots keep their single default row):
        # the table is drawn once, here, and the default row -- what a lookup
        # serves when it serves no stored row -- is default_value_no_permission
        io = opt.init_option if _primary is None else None
        self._init_table_host = None
        self._init_table_dev = None
        if io is not None:
            self._init_table_host = _init_table_host(io, initializer, self.dim, host_dtype, name)
            default = _default_row(io.default_value_no_permission, self.dim, self.device,
                                   host_dtype)
        else:
            default = _default_row(initializer, self.dim, self.device, host_dtype)
        self._default_host = default.to(torch.bfloat16) if bf16 else default
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            if _primary is None:
                cfg = _lib.DrEvConfig()
                cfg.dim = self.dim
                cfg.capacity = int(capacity)
                cfg.steps_to_live = self.steps_to_live
                cfg.filter_freq = self.filter_freq
                cfg.max_element_size = int(getattr(f, "max_element_size", 0) or 0)
                cfg.false_positive_probability = float(
                    getattr(f, "false_positive_probability", -1.0))
                cfg.counter_bits = int(getattr(f, "counter_bits", 64) or 64)
                cfg.layout = 1 if (self.filter_freq or self.steps_to_live) else 0
                cfg.value_bits = {torch.float64: 64, torch.bfloat16: 16}.get(self.value_dtype, 32)
                check(lib().dr_ev_create(C.byref(cfg), default.data_ptr(), C.byref(h)))
                if self._init_table_host is not None:
                    rc = lib().dr_ev_set_init_table(h, self._init_table_host.data_ptr(),
                                                    self._init_table_host.shape[0],
                                                    stream_handle(self.device))
                    if rc:
                        _release_handle(h)
                        check(rc)
            else:
                check(lib().dr_ev_create_slot(_primary._h, _slot_index, default.data_ptr(),
                                              C.byref(h)))
        self._h = h
        self._slots = {}
        self._next_slot = 1

    # -- lifecycle ---------------------------------------------------------
    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _release_handle(self._h)
                self._h = None
            if getattr(self, "_tier", None):    # host memory only: no device call
                lib().dr_host_tier_destroy(self._tier)
                self._tier = None
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def resource(self):
        """The EV as an op input (torch_ops): a host int64[1] tensor holding
        the library handle, TF's DT_RESOURCE scalar (host memory).  Ops that
        change the EV list it in mutates_args."""
        r = getattr(self, "_resource", None)
        if r is None:
            r = torch.tensor([self._h.value], dtype=torch.int64)
            self._resource = r
        return r

    def is_primary(self):
        return self._primary is None

    def slot(self, name, initializer):
        """Slot EV sharing this EV's key space (slot_creator.py:82-117)."""
        if name not in self._slots:
            idx = self._next_slot
            self._next_slot += 1
            self._slots[name] = EmbeddingVariable(self.name + "/" + name, self.dim, initializer,
                                                  device=self.device, _primary=self,
                                                  _slot_index=idx, key_dtype=self.key_dtype)
        return self._slots[name]

    def get_shape(self):
        return (None, self.dim)

    @property
    def default_value(self):
        return self._default_host.to(self.device)

    @property
    def init_table(self):
        """The [default_value_dim, dim] init table in the value dtype (device),
        as the kernels read it; None without an init_option."""
        if self._init_table_host is None:
            return None
        if self._init_table_dev is None:
            self._init_table_dev = self._init_table_host.to(self.value_dtype).to(self.device)
        return self._init_table_dev

    def draws_defaults_per_call(self):
        """A callable initializer without an init_option: every lookup draws a
        fresh [N, D] default block with torch (_defaults_for)."""
        return callable(self.initializer) and self._init_table_host is None

    def pool(self):
        """Base pointer of this EV's value rows (device)."""
        return lib().dr_ev_pool(self._h)

    @property
    def is_bf16(self):
        return self.value_dtype == torch.bfloat16

    @property
    def row_words(self):
        """32-bit words per value row (the kernels' row stride): dim, or
        dim / 2 for a bf16 EV."""
        return self.dim // 2 if self.is_bf16 else self.dim

    # -- ops -----------------------------------------------------------------
    def _defaults_for(self, n, ev_init_value):
        if ev_init_value is not None:
            return torch.as_tensor(ev_init_value, dtype=self.value_dtype,
                                   device=self.device).expand(n, self.dim).contiguous()
        if self.draws_defaults_per_call():
            v = self.initializer((n, self.dim))
            return torch.as_tensor(v, dtype=self.value_dtype, device=self.device).reshape(
                n, self.dim).contiguous()
        return None

    def sparse_read(self, indices, counts=None, ev_init_value=None, name=None, read_only=False):
        """KvResourceGather / KvResourceGatherV1 (kv_variable_ops.py:644-664),
        int32 or int64 ids, float32 or float64 rows per the EV's dtypes.

        read_only (or inside read_only_lookups()): EmbeddingVar::Lookup, the
        inference mode -- an id that is absent, not admitted by the filter or
        untouched in this column reads ev_init_value, else the EV's stored
        default row; nothing is created or counted (`counts` is unused) and a
        callable initializer is not called."""
        if read_only or read_only_active():
            return self._sparse_read_readonly(indices, ev_init_value)
        if (self._primary or self)._tier_n:
            self.promote(indices)
        i32 = indices.dtype == torch.int32
        ids = indices.reshape(-1).to(torch.int32 if i32 else torch.int64).contiguous()
        n = ids.numel()
        out = torch.empty((n, self.dim), dtype=self.value_dtype, device=self.device)
        if n == 0:
            return out.reshape(tuple(indices.shape) + (self.dim,))
        dflt = self._defaults_for(n, ev_init_value)
        cnt = None if counts is None else counts.reshape(-1).to(torch.int32).contiguous()
        if i32:
            wsb = lib().dr_ev_gather_i32_workspace_size(n)
            ws = workspace(wsb, self.device)
            check(lib().dr_ev_gather_i32(self._h, ptr(ids), n, ptr(dflt), ptr(cnt), ptr(out),
                                         ptr(ws), wsb, stream_handle(self.device)))
        else:
            wsb = lib().dr_ev_gather_workspace_size(n)
            ws = workspace(wsb, self.device)
            check(lib().dr_ev_gather(self._h, ptr(ids), n, ptr(dflt), ptr(cnt), ptr(out), ptr(ws),
                                     wsb, stream_handle(self.device)))
        from .ops import _post
        _post(self.device)
        return out.reshape(tuple(indices.shape) + (self.dim,))

    def _sparse_read_readonly(self, indices, ev_init_value=None, defaults=None):
        # (the C entry takes int64 keys: int32 ids are widened here)
        ids = indices.reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        n = ids.numel()
        if n and (self._primary or self)._tier_n and _capturing():
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "a read-only lookup of an HBM_DRAM EmbeddingVariable "
                "whose host tier holds keys cannot be captured in a graph: the rows of the ids "
                "the tier holds are read on the host at every call (run the lookup outside the "
                "capture, or capture while the tier is empty)")
        out = torch.empty((n, self.dim), dtype=self.value_dtype, device=self.device)
        if n:
            if defaults is None and ev_init_value is not None:
                defaults = torch.as_tensor(ev_init_value, dtype=self.value_dtype,
                                           device=self.device).expand(n, self.dim).contiguous()
            check(lib().dr_ev_gather_readonly(self._h, ptr(ids), n, ptr(defaults), ptr(out),
                                              stream_handle(self.device)))
            from .ops import _post
            _post(self.device)
            p = self._primary or self
            if p._tier_n:       # demoted keys are served their rows from the host tier
                with p._lock:
                    self._tier_patch_readonly(ids, out)
        return out.reshape(tuple(indices.shape) + (self.dim,))

    def find(self, keys, n_dev=None):
        """Read-only resolve of keys to rows: -(i+1) = serve the default for
        key i (absent, not admitted, or this column untouched).  The EV is
        left exactly as it was.  HBM only: a key in the host tier is absent."""
        keys = keys.reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        n = keys.numel()
        rows = torch.empty(n, dtype=torch.int64, device=self.device)
        handles = (C.c_void_p * 1)(self._h.value)
        koff = (C.c_int64 * 2)(0, n)
        nd = None if n_dev is None else (C.c_void_p * 1)(n_dev.data_ptr())
        check(lib().dr_ev_find_grouped(handles, 1, ptr(keys), koff, nd, ptr(rows),
                                       stream_handle(self.device)))
        return rows

    def resolve(self, keys, n_dev=None, counts=None, defaults=None):
        """Insert-on-miss resolve of (unique) keys to rows; -(i+1) = default row i."""
        keys = keys.reshape(-1).to(torch.int64).contiguous()
        if (self._primary or self)._tier_n:
            promote_grouped([self], [keys], [n_dev])
        return self._resolve(keys, n_dev, counts, defaults)

    def _resolve(self, keys, n_dev, counts, defaults):
        """resolve() of contiguous int64 keys, without the promotion (the
        grouped lookups promote once for all their features)."""
        n = keys.numel()
        rows = torch.empty(n, dtype=torch.int64, device=self.device)
        wsb = lib().dr_ev_resolve_workspace_size(n)
        ws = workspace(wsb, self.device)
        check(lib().dr_ev_resolve(self._h, ptr(keys), n, ptr(n_dev), ptr(defaults), ptr(counts),
                                  ptr(rows), ptr(ws), wsb, stream_handle(self.device)))
        return rows

    def insert(self, keys, values, versions=None, freqs=None):
        """KvResourceInsert (core/ops/kv_variable_ops.cc:478-492) with
        EmbeddingVar::Import semantics: existing rows are kept."""
        return self._import(keys, values, versions, freqs, 0, 0)

    def import_partitioned(self, keys, values, versions, freqs, partition_id, partition_num):
        """KvResourceImportV2 restore filter key % 1000 % partition_num == id."""
        return self._import(keys, values, versions, freqs, partition_id, partition_num)

    def _import(self, keys, values, versions, freqs, pid, pnum):
        i32 = keys.dtype == torch.int32
        k = keys.reshape(-1).to(device=self.device,
                                dtype=torch.int32 if i32 else torch.int64).contiguous()
        if (self._primary or self)._tier_n:
            self.promote(k)     # an insert keeps the row of a key the model holds
        v = values.reshape(k.numel(), self.dim).to(device=self.device,
                                                   dtype=self.value_dtype).contiguous()
        ver = None if versions is None else versions.to(device=self.device,
                                                        dtype=torch.int64).contiguous()
        fr = None if freqs is None else freqs.to(device=self.device, dtype=torch.int64).contiguous()
        fn = lib().dr_ev_insert_i32 if i32 else lib().dr_ev_insert
        check(fn(self._h, ptr(k), k.numel(), ptr(v), ptr(ver), ptr(fr), pid, pnum,
                 stream_handle(self.device)))

    def insert_synthetic(self, key_begin, n, seed, key_stride=1):
        """Insert keys key_begin + i*key_stride, i < n, rows synth(seed, key, col)."""
        check(lib().dr_ev_insert_synthetic(self._h, int(key_begin), int(key_stride), int(n),
                                           int(seed), stream_handle(self.device)))

    def total_count(self):
        """KvVariableShape: [num keys, dim].  On a tiered key space the keys in
        HBM only (tier_count() has the host tier's)."""
        n = C.c_int64(0)
        check(lib().dr_ev_size(self._h, C.byref(n), stream_handle(self.device)))
        return torch.tensor([n.value, self.dim], dtype=torch.int64)

    def export(self):
        """KvResourceExport -> (keys, values, versions, freqs), keys ascending
        (keys in the EV's key dtype, values in its value dtype)."""
        m = C.c_int64(0)
        st = stream_handle(self.device)
        check(lib().dr_ev_export(self._h, None, None, None, None, 0, C.byref(m), st))
        M = m.value
        keys = torch.empty(M, dtype=self.key_dtype, device=self.device)
        vals = torch.empty((M, self.dim), dtype=self.value_dtype, device=self.device)
        vers = torch.empty(M, dtype=torch.int64, device=self.device)
        frqs = torch.empty(M, dtype=torch.int64, device=self.device)
        fn = lib().dr_ev_export_i32 if self.key_dtype == torch.int32 else lib().dr_ev_export
        check(fn(self._h, ptr(keys), ptr(vals), ptr(vers), ptr(frqs), M, C.byref(m), st))
        n = m.value
        if self.steps_to_live == 0:
            vers = vers[:0]
        if self.filter_freq == 0:
            frqs = frqs[:0]
        p = self._primary or self
        if p._tier_n:
            return self._export_merged(keys[:n], vals[:n], vers, frqs)
        return keys[:n], vals[:n], vers, frqs

    def _export_merged(self, keys, vals, vers, frqs):
        """export() of a tiered key space: HBM's entries and the host tier's
        under the same rule (the primary's and this column's first-touch bit),
        as one list, keys ascending."""
        import numpy as np
        p = self._primary or self
        col = self._slot_index
        with p._lock:
            tk, tv, tve, tfr, tcm = p._tier_export(columns=(col,))
        need = np.uint32(1 | (1 << col))
        sel = np.nonzero((tcm & need) == need)[0]
        if col >= p._tier_ncols or sel.size == 0:
            return keys, vals, vers, frqs
        dev = self.device
        rows = torch.from_numpy(tv[col][sel]).to(dev).view(self.value_dtype).reshape(-1, self.dim)
        k2 = torch.cat([keys, torch.from_numpy(tk[sel]).to(dev)])
        k2, order = torch.sort(k2)
        v2 = torch.cat([vals, rows]).index_select(0, order)
        if vers.numel() or self.steps_to_live:
            vers = torch.cat([vers, torch.from_numpy(tve[sel]).to(dev)]).index_select(0, order)
        if frqs.numel() or self.filter_freq:
            frqs = torch.cat([frqs, torch.from_numpy(tfr[sel]).to(dev)]).index_select(0, order)
        return k2, v2, vers, frqs

    # -- incremental checkpoints (build-defined) -----------
    def _require_int64_keys(self, what):
        if self.key_dtype != torch.int64:
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "%s needs an int64-key EmbeddingVariable (%s has %s keys)"
                % (what, self.name, self.key_dtype))

    def track_updates(self, on=True, by_row=False):
        """Start (or stop) recording which keys of the key space this EV
        shares with its slots are updated: one bit per row, set by
        mark_updated -- the optimizers' apply_gradients marks the gradient's
        indices, RecordSparseIndices' role -- and read by export_updated.
        by_row: apply_gradients marks from the rows the forward resolved
        (mark_updated_rows) wherever a pending gradient carries them -- no
        probe of the key table, and a fused SGD group stays fused; the same
        bits.  The flag holds until the next track_updates call.  On a tiered
        key space (StorageOption(..., incremental=True)) the demoted keys carry
        their bit in the host store; turning tracking off, or on while it was
        off, drops those too."""
        self._require_int64_keys("track_updates")
        self._refuse_tiered("track_updates")
        p = self._primary or self
        fresh = not (on and p._tracking)    # (on while on keeps the marks, as the device side)
        check(lib().dr_ev_track_updates(self._h, 1 if on else 0, stream_handle(self.device)))
        if fresh:
            p._tier_clear_updated()
        p._tracking = bool(on)
        p._tracking_by_row = bool(on) and bool(by_row)

    def tracking_updates(self):
        """Whether this EV's key space records updates (the host-side mirror
        of dr_ev_tracking_updates: no library call on the per-step path)."""
        return (self._primary or self)._tracking

    def tracking_by_row(self):
        """Whether the key space tracks updates and apply_gradients marks
        them by row (track_updates(by_row=True))."""
        return (self._primary or self)._tracking_by_row

    def mark_updated(self, keys, num_valid=None):
        """Mark `keys` (the first num_valid of them: device int64[1]) as
        updated.  Keys that are absent or whose primary row is untouched are
        ignored, nothing is created; a no-op while tracking is off."""
        mark_updated_grouped([self], [keys], [num_valid])

    def mark_updated_rows(self, rows, num_valid=None):
        """mark_updated by row: `rows` (the first num_valid of them) are rows
        a lookup of this EV resolved (find(), a forward's recorded rows), with
        no compact(), remove() or restore since.  Negative rows and rows past
        the row capacity are ignored; a no-op while tracking is off."""
        mark_updated_rows_grouped([self], [rows], [num_valid])

    def updated_count(self):
        """Number of marked rows, plus the marked keys the host tier holds: an
        upper bound on len(export_updated()[0])."""
        n = C.c_int64(0)
        check(lib().dr_ev_updated_count(self._h, C.byref(n), stream_handle(self.device)))
        p = self._primary or self
        if p._tier_n:       # the marked keys the host tier holds
            with p._lock:
                t = C.c_int64(0)
                check(lib().dr_host_tier_count_masked(p._tier, _lib.TIER_UPDATED, C.byref(t)))
            return n.value + t.value
        return n.value

    def export_updated(self):
        """export() narrowed to the marked keys: (keys, values, versions,
        freqs), keys ascending.  Marks are left in place (clear_updated).  On
        a tiered key space the marked keys of both tiers, as export()."""
        if (self._primary or self)._tier_n:
            return self._export_updated_merged(*self._export_updated_hbm())
        return self._export_updated_hbm()

    def _export_updated_merged(self, keys, vals, vers, frqs):
        """export_updated() of a tiered key space: HBM's marked entries and
        the host tier's entries that carry the update bit, under the rule HBM
        applies (the primary's and this column's first-touch bit), as one
        list, keys ascending.  Only the flagged entries are read out of the
        store (dr_host_tier_export_masked), not the tier."""
        import numpy as np
        p = self._primary or self
        col = self._slot_index
        if col >= p._tier_ncols:    # a column made after the store: untouched for its keys
            return keys, vals, vers, frqs
        mask = _lib.TIER_UPDATED | 1 | (1 << col)
        with p._lock:
            m = C.c_int64(0)
            check(lib().dr_host_tier_count_masked(p._tier, mask, C.byref(m)))
            M = m.value
            if M == 0:
                return keys, vals, vers, frqs
            tk, tve, tfr = np.empty(M, np.int64), np.empty(M, np.int64), np.empty(M, np.int64)
            tv = np.empty((M, self._col_bytes(self)), np.uint8)
            vptr = (C.c_void_p * p._tier_ncols)()
            vptr[col] = tv.ctypes.data
            check(lib().dr_host_tier_export_masked(p._tier, mask, tk.ctypes.data, vptr,
                                                   tve.ctypes.data, tfr.ctypes.data, None, M,
                                                   C.byref(m)))
            assert m.value == M, (m.value, M)
        dev = self.device
        rows = torch.from_numpy(tv).to(dev).view(self.value_dtype).reshape(-1, self.dim)
        k2 = torch.cat([keys, torch.from_numpy(tk).to(dev)])
        k2, order = torch.sort(k2)
        v2 = torch.cat([vals, rows]).index_select(0, order)
        if vers.numel() or self.steps_to_live:
            vers = torch.cat([vers, torch.from_numpy(tve).to(dev)]).index_select(0, order)
        if frqs.numel() or self.filter_freq:
            frqs = torch.cat([frqs, torch.from_numpy(tfr).to(dev)]).index_select(0, order)
        return k2, v2, vers, frqs

    def _export_updated_hbm(self):
        self._require_int64_keys("export_updated")
        m = C.c_int64(0)
        st = stream_handle(self.device)
        # the marked-row count bounds the export: the buffers are sized by it
        # and the slot table is scanned once, not once more for the count
        check(lib().dr_ev_updated_count(self._h, C.byref(m), st))
        M = m.value
        keys = torch.empty(M, dtype=torch.int64, device=self.device)
        vals = torch.empty((M, self.dim), dtype=self.value_dtype, device=self.device)
        vers = torch.empty(M, dtype=torch.int64, device=self.device)
        frqs = torch.empty(M, dtype=torch.int64, device=self.device)
        if M:
            check(lib().dr_ev_export_updated(self._h, ptr(keys), ptr(vals), ptr(vers), ptr(frqs),
                                             M, C.byref(m), st))
        n = m.value
        if self.steps_to_live == 0:
            vers = vers[:0]
        if self.filter_freq == 0:
            frqs = frqs[:0]
        return keys[:n], vals[:n], vers[:n], frqs[:n]

    def clear_updated(self):
        check(lib().dr_ev_clear_updated(self._h, stream_handle(self.device)))
        (self._primary or self)._tier_clear_updated()

    def _tier_clear_updated(self):
        """Drops the update bit of every key the host store holds (primary)."""
        if self._tier is not None:
            with self._lock:
                check(lib().dr_host_tier_clear_bits(self._tier, _lib.TIER_UPDATED, None))

    def _tier_log_removed(self, hk):
        """The keys (host numpy) the host tier dropped join the removal log of
        the key space, as the keys HBM drops do (a no-op while not logging)."""
        if hk.size:
            dk = torch.from_numpy(hk).to(self.device)
            check(lib().dr_ev_log_removed(self._h, ptr(dk), dk.numel(),
                                          stream_handle(self.device)))

    def upsert(self, keys, values, versions=None, freqs=None):
        """insert() that OVERWRITES the rows of keys already present (insert
        keeps them): how a delta is applied.  Keys must be distinct."""
        return self._upsert(keys, values, versions, freqs, 0, 0)

    def _upsert(self, keys, values, versions, freqs, pid, pnum):
        self._require_int64_keys("upsert")
        k = keys.reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        if (self._primary or self)._tier_n:
            self.promote(k)     # the other columns, version rules and freq of the key stay
        v = values.reshape(k.numel(), self.dim).to(device=self.device,
                                                   dtype=self.value_dtype).contiguous()
        ver = None if versions is None else versions.to(device=self.device,
                                                        dtype=torch.int64).contiguous()
        fr = None if freqs is None else freqs.to(device=self.device, dtype=torch.int64).contiguous()
        check(lib().dr_ev_upsert(self._h, ptr(k), k.numel(), ptr(v), ptr(ver), ptr(fr), pid, pnum,
                                 stream_handle(self.device)))

    def key_meta(self, keys):
        """(freq, version, has_row) of keys, host numpy (tests/debug).  HBM
        only: a key in the host tier has no row."""
        import numpy as np
        k = np.ascontiguousarray(keys, dtype=np.int64)
        n = k.shape[0]
        fr = np.zeros(n, np.int64)
        ve = np.zeros(n, np.int64)
        hr = np.zeros(n, np.int32)
        check(lib().dr_ev_key_meta(self._h, k.ctypes.data, n, fr.ctypes.data, ve.ctypes.data,
                                   hr.ctypes.data, stream_handle(self.device)))
        return fr, ve, hr.astype(bool)

    def reserve(self, extra):
        check(lib().dr_ev_reserve(self._h, int(extra), stream_handle(self.device)))

    def shrink(self, global_step=0):
        """EmbeddingVar::Shrink (embedding_var.h:264-313) on the key space this
        EV shares with its slots: by L2 weight when l2_weight_threshold != -1,
        else by global step when steps_to_live > 0.  Returns keys removed."""
        p = self._primary or self
        n = C.c_int64(0)
        check(lib().dr_ev_shrink(p._h, int(global_step), p.l2_weight_threshold, C.byref(n),
                                 stream_handle(self.device)))
        if p._tier_n and p.steps_to_live > 0:   # the age rule on the host tier's keys too
            import numpy as np
            gone = None
            with p._lock:
                t = C.c_int64(0)
                if p._tier_incremental and p.tracking_removals():
                    # the removal log gets the tier's victims as it got HBM's
                    gone = np.empty(p._tier_n, np.int64)
                    check(lib().dr_host_tier_shrink_keys(p._tier, int(global_step),
                                                         p.steps_to_live, gone.ctypes.data,
                                                         gone.size, C.byref(t)))
                else:
                    check(lib().dr_host_tier_shrink(p._tier, int(global_step), p.steps_to_live,
                                                    C.byref(t)))
                p._tier_n -= t.value
            if gone is not None:
                p._tier_log_removed(gone[:t.value])
            return n.value + t.value
        return n.value

    def compact(self):
        """Row compaction (dr_ev_compact) of the key space this EV shares with
        its slots: the live rows above the live count move into the rows that
        shrink() left behind and the tail is free for new keys.  Returns the
        rows reclaimed.  Row indices handed out earlier are invalid afterwards,
        so a queued gradient (pending_grads of the primary or a slot EV: it
        may hold a forward's recorded rows) is refused: apply it first."""
        p = self._primary or self
        for ev in [p] + list(p._slots.values()):
            if ev.pending_grads:
                raise _lib.InvalidArgumentError(
                    _lib.INVALID_ARGUMENT, "compact: %s has %d pending gradient(s), which may "
                    "hold row indices; apply_gradients first" % (ev.name, len(ev.pending_grads)))
        n = C.c_int64(0)
        check(lib().dr_ev_compact(p._h, C.byref(n), stream_handle(self.device)))
        return n.value

    def rows_allocated(self):
        """Rows allocated in the key space (the device row counter):
        total_count()[0] plus the rows of evicted keys not yet compacted.
        HBM only: the host tier's keys hold no row."""
        n = C.c_int64(0)
        check(lib().dr_ev_rows_allocated(self._h, C.byref(n), stream_handle(self.device)))
        return n.value

    # -- keyed removal and the removal log (build-defined) --
    def remove(self, keys):
        """Remove `keys` from the key space this EV shares with its slots
        (dr_ev_remove, through the primary as shrink()).  Absent keys are
        ignored, duplicates count once; returns the distinct keys removed.
        Rows stay allocated until compact().  A call costs one pass over the
        slot table whatever len(keys) is: batch.  A queued gradient
        (pending_grads of the primary or a slot EV) is refused, as in
        compact(): its recorded rows would refer to dead keys."""
        self._require_int64_keys("remove")
        p = self._primary or self
        for ev in [p] + list(p._slots.values()):
            if ev.pending_grads:
                raise _lib.InvalidArgumentError(
                    _lib.INVALID_ARGUMENT, "remove: %s has %d pending gradient(s), which may "
                    "hold rows of the keys; apply_gradients first" % (ev.name, len(ev.pending_grads)))
        k = keys.reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        n = C.c_int64(0)
        check(lib().dr_ev_remove(p._h, ptr(k), k.numel(), C.byref(n), stream_handle(self.device)))
        if p._tier_n:       # a key lives in one tier: the counts add up
            if p._tier_incremental and p.tracking_removals():
                with p._lock:
                    gone = p._tier_remove_keys(k)
                p._tier_log_removed(gone)   # the tier's victims join the log as HBM's did
                return n.value + gone.size
            with p._lock:
                return n.value + p._tier_remove(k)
        return n.value

    def shrink_to(self, max_keys, policy="lru"):
        """Key budget (dr_ev_shrink_to, through the primary as shrink()): when
        the key space this EV shares with its slots holds more than `max_keys`
        keys, the coldest go -- the first total_count() - max_keys by (version,
        key) for "lru" (version -1, not yet stamped, counts as newest) or by
        (freq, key) for "lfu" -- exactly as remove() of those keys: rows stay
        allocated until compact() and the removal log gets them.  At or under
        the budget nothing changes.  Returns the keys removed.  A queued
        gradient (pending_grads of the primary or a slot EV) is refused, as in
        remove(): its recorded rows would refer to dead keys.  HBM only, also
        on a tiered key space: the victims are dropped, not demoted
        (demote_to), and the host tier is not looked at."""
        self._require_int64_keys("shrink_to")
        if policy not in _EVICT_POLICIES:
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "shrink_to: policy is 'lru' or 'lfu', not %r" % (policy,))
        p = self._primary or self
        for ev in [p] + list(p._slots.values()):
            if ev.pending_grads:
                raise _lib.InvalidArgumentError(
                    _lib.INVALID_ARGUMENT, "shrink_to: %s has %d pending gradient(s), which may "
                    "hold rows of the keys; apply_gradients first"
                    % (ev.name, len(ev.pending_grads)))
        n = C.c_int64(0)
        check(lib().dr_ev_shrink_to(p._h, int(max_keys), _EVICT_POLICIES[policy], C.byref(n),
                                    stream_handle(self.device)))
        return n.value

    def track_removals(self, on=True):
        """Start (with an empty log) or stop logging the keys that shrink()
        and remove() drop from the key space this EV shares with its slots;
        save_incremental writes the log into the delta."""
        self._require_int64_keys("track_removals")
        self._refuse_tiered("track_removals")
        check(lib().dr_ev_track_removals(self._h, 1 if on else 0, stream_handle(self.device)))

    def tracking_removals(self):
        return lib().dr_ev_tracking_removals(self._h) == 1

    def removed_count(self):
        """Entries in the removal log: an upper bound on len(export_removed())."""
        n = C.c_int64(0)
        check(lib().dr_ev_removed_count(self._h, C.byref(n), stream_handle(self.device)))
        return n.value

    def export_removed(self):
        """The distinct logged keys, ascending (device int64).  The log is not
        filtered against the map and stays in place (clear_removed)."""
        self._require_int64_keys("export_removed")
        st = stream_handle(self.device)
        m = C.c_int64(0)
        check(lib().dr_ev_removed_count(self._h, C.byref(m), st))
        keys = torch.empty(m.value, dtype=torch.int64, device=self.device)
        if m.value:
            check(lib().dr_ev_export_removed(self._h, ptr(keys), m.value, C.byref(m), st))
        return keys[:m.value]

    def clear_removed(self):
        check(lib().dr_ev_clear_removed(self._h, stream_handle(self.device)))

    # -- HBM + host-DRAM tier (build-defined) ---------------
    @property
    def tiered(self):
        """Whether the key space this EV shares with its slots has a host-DRAM
        tier (StorageOption(StorageType.HBM_DRAM) on the primary)."""
        return (self._primary or self)._tiered

    def tier_count(self):
        """Keys held in the host-DRAM tier (0 for an untiered EV).  Host side."""
        return (self._primary or self)._tier_n

    def _refuse_tiered(self, what):
        # a demoted row's update bit, and a demotion that is no removal, would
        # have to travel with the key: incremental checkpoints of a tiered key
        # space are built only for StorageOption(..., incremental=True)
        if self.tiered and not (self._primary or self)._tier_incremental:
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "%s: %s has a host-DRAM tier (StorageType.HBM_DRAM); "
                "incremental checkpoints of a tiered key space are not supported"
                % (what, self.name))

    def _require_tiered(self, what):
        if not self.tiered:
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "%s needs StorageOption(StorageType.HBM_DRAM) (%s)"
                % (what, self.name))

    def _columns(self):
        """The key space's columns by index (None where no slot EV exists)."""
        p = self._primary or self
        cols = [None] * p._next_slot
        cols[0] = p
        for ev in p._slots.values():
            cols[ev._slot_index] = ev
        return cols

    @staticmethod
    def _col_bytes(ev):
        return 0 if ev is None else ev.dim * torch.empty(0, dtype=ev.value_dtype).element_size()

    def _tier_store(self, cols):
        """The primary's host store, made for (at least) the columns `cols`.
        Slots created after the store move it to a wider one: their column is
        untouched for every key it holds."""
        n = len(cols)
        if self._tier is not None and self._tier_ncols >= n:
            return self._tier
        t = C.c_void_p()
        cb = (C.c_int64 * n)(*[self._col_bytes(ev) for ev in cols])
        check(lib().dr_host_tier_create(n, cb, self._tier_n, C.byref(t)))
        if self._tier is not None:
            k, vals, ve, fr, cm = self._tier_export(self._tier_ncols)
            ptrs = (C.c_void_p * n)(*[v.ctypes.data if v is not None else None for v in vals]
                                    + [None] * (n - self._tier_ncols))
            check(lib().dr_host_tier_put(t, k.ctypes.data, k.size, ptrs, ve.ctypes.data,
                                         fr.ctypes.data, cm.ctypes.data))
            check(lib().dr_host_tier_destroy(self._tier))
        self._tier, self._tier_ncols = t, n
        return t

    def _tier_export(self, ncols=None, columns=None):
        """(keys, [values per column], versions, freqs, colmask) of the store,
        host numpy, keys ascending; values only of `columns` (default: all)."""
        import numpy as np
        ncols = self._tier_ncols if ncols is None else ncols
        cols = self._columns()
        m = self._tier_n
        k = np.empty(m, np.int64)
        ve, fr, cm = np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.uint32)
        vals = [np.empty((m, self._col_bytes(cols[c])), np.uint8)
                if cols[c] is not None and (columns is None or c in columns) else None
                for c in range(ncols)]
        ptrs = (C.c_void_p * max(ncols, 1))(*[v.ctypes.data if v is not None else None
                                              for v in vals])
        got = C.c_int64(0)
        check(lib().dr_host_tier_export(self._tier, k.ctypes.data, ptrs, ve.ctypes.data,
                                        fr.ctypes.data, cm.ctypes.data, m, C.byref(got)))
        assert got.value == m, (got.value, m)
        return k, vals, ve, fr, cm

    def demote_to(self, max_keys=None, policy=None, compact=True):
        """Moves the coldest keys of the key space out of HBM into the
        host-DRAM tier until HBM holds at most `max_keys` (default: the
        KeyBudgetEvict's): exactly shrink_to's victims, by `policy`, each with
        every column's row, its version, freq and first-touch bits, so that
        promote() puts it back bit for bit.  The removal log does not get
        them: a demoted key stays in the model.  compact: ends in compact(),
        which gives the victims' rows back.  Returns the keys demoted.  A
        queued gradient is refused, as in remove().  Call it between steps
        (after apply_gradients, before the next forward): a forward whose
        backward has not run has queued nothing yet, and its gradient would
        re-create a key demoted in between as a fresh row."""
        import numpy as np
        self._require_tiered("demote_to")
        p = self._primary or self
        max_keys = p.max_keys if max_keys is None else int(max_keys)
        policy = p.policy if policy is None else policy
        if policy not in _EVICT_POLICIES:
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "demote_to: policy is 'lru' or 'lfu', not %r" % (policy,))
        cols = p._columns()
        for ev in cols:
            if ev is not None and ev.pending_grads:
                raise _lib.InvalidArgumentError(
                    _lib.INVALID_ARGUMENT, "demote_to: %s has %d pending gradient(s), which may "
                    "hold rows of the keys; apply_gradients first"
                    % (ev.name, len(ev.pending_grads)))
        st = stream_handle(p.device)
        pol = _EVICT_POLICIES[policy]
        m = C.c_int64(0)
        check(lib().dr_ev_demote_to(p._h, max_keys, pol, None, None, 0, None, None, None, 0,
                                    C.byref(m), st))
        E = m.value
        if E:
            dev = p.device
            keys = torch.empty(E, dtype=torch.int64, device=dev)
            vers = torch.empty(E, dtype=torch.int64, device=dev)
            frqs = torch.empty(E, dtype=torch.int64, device=dev)
            cmask = torch.empty(E, dtype=torch.int32, device=dev)
            vals = [None if ev is None else torch.empty((E, ev.dim), dtype=ev.value_dtype,
                                                        device=dev) for ev in cols]
            n = len(cols)
            vptr = (C.c_void_p * n)(*[ptr(v) for v in vals])
            check(lib().dr_ev_demote_to(p._h, max_keys, pol, ptr(keys), vptr, n, ptr(vers),
                                        ptr(frqs), ptr(cmask), E, C.byref(m), st))
            assert m.value == E, (m.value, E)
            hk, hv, hf, hc = keys.cpu().numpy(), vers.cpu().numpy(), frqs.cpu().numpy(), \
                np.ascontiguousarray(cmask.cpu().numpy().view(np.uint32))
            hvals = [None if v is None else v.contiguous().view(torch.uint8).cpu().numpy()
                     for v in vals]
            with p._lock:
                t = p._tier_store(cols)
                hptr = (C.c_void_p * p._tier_ncols)(*(
                    [None if v is None else v.ctypes.data for v in hvals]
                    + [None] * (p._tier_ncols - n)))
                check(lib().dr_host_tier_put(t, hk.ctypes.data, E, hptr, hv.ctypes.data,
                                             hf.ctypes.data, hc.ctypes.data))
                p._tier_n += E
        if compact:
            self.compact()
        return E

    def promote(self, keys):
        """Brings the keys among `keys` that the host-DRAM tier holds back into
        HBM, exactly as they were demoted (every column's row where it had been
        touched, version, freq, first-touch bits), and drops them from the
        tier.  Keys in HBM already, and keys in neither tier, are left alone.
        Returns the keys promoted.  With an empty tier, or on an untiered EV,
        nothing is launched."""
        p = self._primary or self
        if not p._tier_n:
            return 0
        return promote_grouped([p], [keys])

    def _tier_remove(self, k):
        """remove() on the tier's side; returns the keys it dropped."""
        if not self._tier_n:
            return 0
        hk = k.cpu().numpy()
        n = C.c_int64(0)
        check(lib().dr_host_tier_remove(self._tier, hk.ctypes.data, hk.size, C.byref(n)))
        self._tier_n -= n.value
        return n.value

    def _tier_remove_keys(self, k):
        """_tier_remove that returns the dropped keys (host numpy): take with
        erase and no value outputs."""
        import numpy as np
        hk = np.ascontiguousarray(k.cpu().numpy())
        idx = np.empty(hk.size, np.int64)
        hits = C.c_int64(0)
        check(lib().dr_host_tier_take(self._tier, hk.ctypes.data, hk.size, 1, idx.ctypes.data,
                                      None, None, None, None, C.byref(hits)))
        self._tier_n -= hits.value
        return np.ascontiguousarray(hk[idx[:hits.value]])

    def _tier_patch_readonly(self, ids, out):
        """The read-only lookup's second half on a tiered key space: the rows
        of the ids the tier holds go from the store into `out`, under the rules
        HBM applies (this column's and the primary's first-touch bit set, and
        for a Counter filter the stored freq >= filter_freq); neither tier
        changes."""
        import numpy as np
        p = self._primary or self
        hk = ids.cpu().numpy()
        uniq, inv = np.unique(hk, return_inverse=True)
        col = self._slot_index
        nb = self._col_bytes(self)
        hit_idx = np.empty(uniq.size, np.int64)
        rows = np.empty((uniq.size, nb), np.uint8)
        fr, cm = np.empty(uniq.size, np.int64), np.empty(uniq.size, np.uint32)
        vptr = (C.c_void_p * p._tier_ncols)()
        if col < p._tier_ncols:
            vptr[col] = rows.ctypes.data
        hits = C.c_int64(0)
        check(lib().dr_host_tier_take(p._tier, uniq.ctypes.data, uniq.size, 0, hit_idx.ctypes.data,
                                      vptr, None, fr.ctypes.data, cm.ctypes.data, C.byref(hits)))
        h = hits.value
        ok = tier_rows_served(cm[:h], fr[:h], col, p.filter_freq)
        src_of_uniq = np.full(uniq.size, -1, np.int64)
        src_of_uniq[hit_idx[:h][ok]] = np.nonzero(ok)[0]
        src = src_of_uniq[inv.reshape(-1)]
        pos = np.nonzero(src >= 0)[0]
        if pos.size:
            # rows as 32-bit words, whatever the value dtype (dr_rows_scatter moves words)
            block = torch.from_numpy(rows[src[pos]]).to(self.device).view(torch.float32)
            from .ops import rows_scatter
            rows_scatter(block, torch.from_numpy(pos.astype(np.int32)).to(self.device),
                         out.view(torch.float32))
        return h

    def _tier_serve_rows(self, miss):
        """(keys, rows) this column serves read-only out of the host tier for
        the host int64 keys `miss` (duplicates allowed): the keys distinct and
        ascending as signed int64, rows[i] the stored row bytes of keys[i].
        tier_rows_served decides; neither tier changes (take, erase=0)."""
        import numpy as np
        p = self._primary or self
        col = self._slot_index
        nb = self._col_bytes(self)
        none = np.empty(0, np.int64), np.empty((0, nb), np.uint8)
        with p._lock:
            if not p._tier_n or col >= p._tier_ncols or miss.size == 0:
                return none
            miss = np.ascontiguousarray(miss)
            # which of them the store holds (never-seen ids are most of a batch's
            # misses): the row buffer below is sized by the hits alone
            idx = np.empty(miss.size, np.int64)
            hits = C.c_int64(0)
            check(lib().dr_host_tier_take(p._tier, miss.ctypes.data, miss.size, 0, idx.ctypes.data,
                                          None, None, None, None, C.byref(hits)))
            if not hits.value:
                return none
            held = np.ascontiguousarray(miss[idx[:hits.value]])
            n = held.size
            rows = np.empty((n, nb), np.uint8)
            fr, cm = np.empty(n, np.int64), np.empty(n, np.uint32)
            vptr = (C.c_void_p * p._tier_ncols)()
            vptr[col] = rows.ctypes.data
            check(lib().dr_host_tier_take(p._tier, held.ctypes.data, n, 0, idx.ctypes.data, vptr,
                                          None, fr.ctypes.data, cm.ctypes.data, C.byref(hits)))
            h = hits.value
        ok = np.nonzero(tier_rows_served(cm[:h], fr[:h], col, p.filter_freq))[0]
        keys = held[idx[:h]][ok]
        order = np.argsort(keys, kind="stable")     # distinct: the sort is np.unique's
        return np.ascontiguousarray(keys[order]), np.ascontiguousarray(rows[:h][ok][order])


def tier_rows_served(colmask, freq, col, filter_freq):
    """Which entries of the host tier a read-only lookup of column `col`
    serves, by the rule HBM applies (RoDesc, ev.hip): the primary's and the
    column's first-touch bit set in the stored colmask -- the other bits,
    DR_TIER_UPDATED among them, do not matter -- and, for a Counter EV
    (filter_freq > 0), the stored freq >= filter_freq.  numpy in, bool mask out."""
    import numpy as np
    need = np.uint32(1 | (1 << int(col)))
    ok = (np.asarray(colmask, np.uint32) & need) == need
    if filter_freq:
        ok &= np.asarray(freq, np.int64) >= int(filter_freq)
    return ok


def _mark_grouped(what, evs, xs, num_valid, launch):
    """The grouping of the two marks: xs[t] (keys or rows), and the optional
    device count num_valid[t], belong to evs[t]; launch(handles, T, flat, koff,
    nd, stream) once per device and MAX_GROUP tables.  EVs whose key space is
    not tracking, and empty inputs, are left out."""
    by_dev = {}
    for t, ev in enumerate(evs):
        if ev.tracking_updates() and xs[t].numel():
            ev._require_int64_keys(what)
            by_dev.setdefault(str(ev.device), []).append(
                (ev, xs[t], None if num_valid is None else num_valid[t]))
    for items in by_dev.values():
        while items:
            chunk, items = items[:_lib.MAX_GROUP], items[_lib.MAX_GROUP:]
            dev, T = chunk[0][0].device, len(chunk)
            ks = [k.reshape(-1).to(device=dev, dtype=torch.int64) for _, k, _ in chunk]
            flat = ks[0].contiguous() if T == 1 else torch.cat(ks)
            koff = (C.c_int64 * (T + 1))()
            for t in range(T):
                koff[t + 1] = koff[t] + ks[t].numel()
            handles = (C.c_void_p * T)(*[ev._h.value for ev, _, _ in chunk])
            nd = (C.c_void_p * T)(*[None if n is None else n.data_ptr() for _, _, n in chunk])
            check(launch(handles, T, ptr(flat), koff, nd, stream_handle(dev)))


def mark_updated_grouped(evs, keys, num_valid=None):
    """mark_updated over several EVs with one launch per device and
    MAX_GROUP tables (dr_ev_mark_updated's grouping): keys[t], and the
    optional device count num_valid[t], belong to evs[t].  EVs whose key
    space is not tracking are left out.  A tracking EV whose host tier holds
    keys also has the ones among keys[t] that the tier holds with the primary
    bit set flagged there, as an untiered table would mark them (a host read
    of the keys: this is the public route, not apply_gradients')."""
    _mark_updated_hbm(evs, keys, num_valid)
    import numpy as np
    for t, ev in enumerate(evs):
        p = getattr(ev, "_primary", None) or ev
        if not (getattr(p, "_tier_n", 0) and ev.tracking_updates() and keys[t].numel()):
            continue
        k = keys[t].reshape(-1)
        if num_valid is not None and num_valid[t] is not None:
            k = k[:int(num_valid[t].item())]
        hk = np.ascontiguousarray(k.to(torch.int64).cpu().numpy())
        with p._lock:
            check(lib().dr_host_tier_or_bits(p._tier, hk.ctypes.data, hk.size, 1,
                                             _lib.TIER_UPDATED, None))


def _mark_updated_hbm(evs, keys, num_valid=None):
    """mark_updated_grouped on the device alone: apply_gradients' route.  The
    keys of a pending gradient were promoted by their forward, so the host
    tier is not consulted -- a tiered EV's step costs what an untiered one's
    does."""
    _mark_grouped("mark_updated", evs, keys, num_valid, lib().dr_ev_mark_updated)


def mark_updated_rows_grouped(evs, rows, num_valid=None):
    """mark_updated_rows over several EVs, grouped as mark_updated_grouped
    (dr_ev_mark_updated_rows, position order): rows[t], and the optional
    device count num_valid[t], belong to evs[t]."""
    _mark_grouped("mark_updated_rows", evs, rows, num_valid,
                  lambda h, T, flat, koff, nd, st:
                  lib().dr_ev_mark_updated_rows(h, T, flat, koff, 0, nd, st))


def _tier_misses(items):
    """dr_ev_missing_keys over `items` = [(primary EV, keys, num_valid or
    None)] of one device, at most MAX_GROUP of them: per item the host numpy
    keys (duplicates kept) that are not in its HBM table.  One launch and one
    host read of the count for the whole group."""
    dev, T = items[0][0].device, len(items)
    ks = [k.reshape(-1).to(device=dev, dtype=torch.int64) for _, k, _ in items]
    flat = ks[0].contiguous() if T == 1 else torch.cat(ks)
    koff = [0]
    for k in ks:
        koff.append(koff[-1] + k.numel())
    total = koff[-1]
    if total == 0:
        return [None] * T
    mk = torch.empty(total, dtype=torch.int64, device=dev)
    mp = torch.empty(total, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    handles = (C.c_void_p * T)(*[ev._h.value for ev, _, _ in items])
    nd = (C.c_void_p * T)(*[None if n is None else n.data_ptr() for _, _, n in items])
    check(lib().dr_ev_missing_keys(handles, T, ptr(flat), (C.c_int64 * (T + 1))(*koff), nd,
                                   ptr(mk), ptr(mp), ptr(cnt), stream_handle(dev)))
    m = int(cnt.item())     # the step's one synchronise
    if m == 0:
        return [None] * T
    hk, hp = mk[:m].cpu().numpy(), mp[:m].cpu().numpy()
    return [hk[(hp >= koff[t]) & (hp < koff[t + 1])] for t in range(T)]


def _tiered_items(evs, keys, num_valid):
    """The (primary, keys, num_valid) of the EVs whose tier holds anything,
    by device; refuses stream capture when there is one."""
    by_dev = {}
    for t, ev in enumerate(evs):
        p = getattr(ev, "_primary", None) or ev
        if getattr(p, "_tier_n", 0) and keys[t].numel():
            by_dev.setdefault(str(p.device), []).append(
                (p, keys[t], None if num_valid is None else num_valid[t]))
    if by_dev:
        _refuse_tier_capture()
    return by_dev


def _refuse_tier_capture():
    if _capturing():
        raise _lib.InvalidArgumentError(
            _lib.INVALID_ARGUMENT, "a lookup of an HBM_DRAM EmbeddingVariable whose host tier "
            "holds keys cannot be captured in a graph: which keys to promote is read on the "
            "host at every call (run the lookup outside the capture, or capture while the "
            "tier is empty)")


def promote_grouped(evs, keys, num_valid=None):
    """promote() over several EVs: keys[t] (the first num_valid[t] of them:
    device int64[1]) belong to evs[t].  One dr_ev_missing_keys per device and
    MAX_GROUP tables finds the keys that are not in HBM; the host store gives
    up the ones it holds (take, erase) and dr_ev_promote re-inserts them.
    EVs without a tier, or with an empty one, are left out: for them nothing
    is launched.  Returns the keys promoted."""
    import numpy as np
    promoted = 0
    for items in _tiered_items(evs, keys, num_valid).values():
        while items:
            chunk, items = items[:_lib.MAX_GROUP], items[_lib.MAX_GROUP:]
            for (p, _, _), miss in zip(chunk, _tier_misses(chunk)):
                if miss is None or miss.size == 0 or not p._tier_n:
                    continue
                with p._lock:
                    cols = p._columns()[:p._tier_ncols]
                    # which misses the store holds (brand-new keys are most of a step's
                    # misses): the row buffers below are sized by the hits alone
                    idx0 = np.empty(miss.size, np.int64)
                    hits = C.c_int64(0)
                    check(lib().dr_host_tier_take(p._tier, miss.ctypes.data, miss.size, 0,
                                                  idx0.ctypes.data, None, None, None, None,
                                                  C.byref(hits)))
                    if not hits.value:
                        continue
                    miss = np.ascontiguousarray(miss[idx0[:hits.value]])
                    n = miss.size
                    ve, fr = np.empty(n, np.int64), np.empty(n, np.int64)
                    cm = np.empty(n, np.uint32)
                    vals = [None if ev is None else np.empty((n, p._col_bytes(ev)), np.uint8)
                            for ev in cols]
                    vptr = (C.c_void_p * p._tier_ncols)(*[None if v is None else v.ctypes.data
                                                          for v in vals])
                    idx = np.empty(n, np.int64)
                    hits = C.c_int64(0)
                    check(lib().dr_host_tier_take(p._tier, miss.ctypes.data, n, 1, idx.ctypes.data,
                                                  vptr, ve.ctypes.data, fr.ctypes.data,
                                                  cm.ctypes.data, C.byref(hits)))
                    h = hits.value
                    if not h:
                        continue
                    p._tier_n -= h
                    dev = p.device
                    dk = torch.from_numpy(miss[idx[:h]]).to(dev)
                    dvals = [None if v is None else torch.from_numpy(v[:h]).to(dev) for v in vals]
                    dptr = (C.c_void_p * p._tier_ncols)(*[ptr(v) for v in dvals])
                    dve, dfr = torch.from_numpy(ve[:h]).to(dev), torch.from_numpy(fr[:h]).to(dev)
                    dcm = torch.from_numpy(cm[:h].view(np.int32)).to(dev)
                    check(lib().dr_ev_promote(p._h, ptr(dk), h, dptr, p._tier_ncols, ptr(dve),
                                              ptr(dfr), ptr(dcm), stream_handle(dev)))
                    promoted += h
    return promoted


def tier_hits(evs, keys, num_valid=None):
    """How many of keys[t] -- distinct per EV -- the host tier of evs[t] holds;
    neither tier changes.  0 without a launch when every tier is empty."""
    import numpy as np
    hits = 0
    for items in _tiered_items(evs, keys, num_valid).values():
        while items:
            chunk, items = items[:_lib.MAX_GROUP], items[_lib.MAX_GROUP:]
            for (p, _, _), miss in zip(chunk, _tier_misses(chunk)):
                if miss is None or miss.size == 0:
                    continue
                h = C.c_int64(0)
                with p._lock:
                    check(lib().dr_host_tier_take(p._tier, miss.ctypes.data, miss.size, 0, None,
                                                  None, None, None, None, C.byref(h)))
                hits += h.value
    return hits


class TierOverlay(object):
    """What the host tier serves for one group's batch (tier_serve_overlay)."""

    def __init__(self, keys, off, blob, row_bytes, miss_keys, miss_pos):
        self.keys = keys              # device int64[M], ascending inside each table's range
        self.off = off                # host prefix, T + 1 entries
        self.blob = blob              # device uint8: the M rows, table after table
        self.row_bytes = row_bytes    # per table
        self.miss_keys = miss_keys    # device: dr_ev_missing_keys' list (m entries)
        self.miss_pos = miss_pos

    def off_array(self):
        return (C.c_int64 * len(self.off))(*self.off)

    def rows(self, t, dtype):
        """Table t's served rows, [n_t, dim] of the EV's value type."""
        b0 = sum((self.off[u + 1] - self.off[u]) * self.row_bytes[u] for u in range(t))
        n = self.off[t + 1] - self.off[t]
        return self.blob[b0:b0 + n * self.row_bytes[t]].view(dtype).view(n, -1)


_ZERO_COUNT = {}


def tier_serve_overlay(evs, keys, num_valid=None, koff=None):
    """The overlay a read-only pooled lookup serves from the host tier, for one
    group: evs[t] (<= MAX_GROUP columns on one device, tiered or not) is looked
    up at keys[t] (the first num_valid[t] of them: device int64[1]) -- or, with
    the host prefix `koff`, at keys[koff[t]:koff[t + 1]] of the one flat device
    tensor `keys`.  One dr_ev_missing_keys and one host read of its count; only
    the keys HBM does not hold come to the host, where each EV's store gives
    the rows it serves (EmbeddingVariable._tier_serve_rows).  None when every
    tier is empty (nothing is launched), when HBM holds the whole batch, or
    when the tier serves none of the missing keys: the lookup then runs as
    without a tier.  Neither tier changes."""
    import numpy as np
    T = len(evs)
    prim = [getattr(ev, "_primary", None) or ev for ev in evs]
    if koff is None:
        dev = prim[0].device
        ks = [k.reshape(-1).to(device=dev, dtype=torch.int64) for k in keys]
        koff = [0]
        for k in ks:
            koff.append(koff[-1] + k.numel())
    else:
        ks = None
    tiered = [bool(getattr(p, "_tier_n", 0)) and koff[t + 1] > koff[t]
              for t, p in enumerate(prim)]
    if not any(tiered):
        return None
    _refuse_tier_capture()
    dev = prim[0].device
    flat = keys if ks is None else (ks[0].contiguous() if T == 1 else torch.cat(ks))
    total = koff[-1]
    mk = torch.empty(total, dtype=torch.int64, device=dev)
    mp = torch.empty(total, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    nd = [None if num_valid is None or num_valid[t] is None else num_valid[t].data_ptr()
          for t in range(T)]
    if not all(tiered):
        # the other tables of the group take no part: a device count of zero
        z = _ZERO_COUNT.get(str(dev))
        if z is None:
            z = _ZERO_COUNT[str(dev)] = torch.zeros(1, dtype=torch.int64, device=dev)
        nd = [n if tiered[t] else z.data_ptr() for t, n in enumerate(nd)]
    handles = (C.c_void_p * T)(*[p._h.value for p in prim])
    ckoff = (C.c_int64 * (T + 1))(*koff)
    check(lib().dr_ev_missing_keys(handles, T, ptr(flat), ckoff, (C.c_void_p * T)(*nd), ptr(mk),
                                   ptr(mp), ptr(cnt), stream_handle(dev)))
    m = int(cnt.item())     # the call's one synchronise
    if m == 0:
        return None
    mk, mp = mk[:m], mp[:m]
    hk, hp = mk.cpu().numpy(), mp.cpu().numpy()
    tab = np.searchsorted(np.asarray(koff[1:], np.int64), hp, side="right")
    okeys, orows, off, nbs = [], [], [0], []
    for t, ev in enumerate(evs):
        nbs.append(ev._col_bytes(ev))
        if tiered[t]:
            k, r = ev._tier_serve_rows(hk[tab == t])
            if k.size:
                okeys.append(k)
                orows.append(r.reshape(-1))
        off.append(sum(x.size for x in okeys))
    if not okeys:
        return None
    return TierOverlay(torch.from_numpy(np.concatenate(okeys)).to(dev), off,
                       torch.from_numpy(np.concatenate(orows)).to(dev), nbs, mk, mp)


def refuse_multihash(evs, what):
    """The sharded engines shard EmbeddingVariables by key; a MultiHashVariable
    has no keys to shard (its two tables are small enough to replicate)."""
    for ev in evs or ():
        if isinstance(ev, MultiHashVariable):
            raise TypeError("%s shards EmbeddingVariables; %s is a MultiHashVariable (look it "
                            "up locally with embedding_lookup_sparse)" % (what, ev.name))


def refuse_tiered_evs(evs, what):
    """For the entry points that read or create keys in HBM without promoting
    (the sharded engines): a tiered EV would be served defaults for the keys
    its host tier holds, so it is refused."""
    refuse_multihash(evs, what)
    refuse_adaptive(evs, what)
    for ev in evs or ():    # (an engine built without local EVs has none to refuse)
        if getattr(ev, "tiered", False):
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "%s does not promote from a host-DRAM tier: %s has "
                "StorageType.HBM_DRAM" % (what, ev.name))


_EV_REGISTRY = {}


def get_embedding_variable(name, embedding_dim, key_dtype=torch.int64, initializer=None,
                           steps_to_live=0, ev_option=None, capacity=1 << 16, device=None,
                           partitioner=None, l2_weight_threshold=-1.0, value_dtype=torch.float32):
    """tf.get_embedding_variable (variable_scope.py:2142-2197).

    With `partitioner=n` (fixed_size_partitioner(num_shards=n)) returns a list
    of n EVs; lookups route key -> shard by key % 1000 % n
    (embedding_ops.py:207-209)."""
    if partitioner is not None and int(partitioner) > 1:
        return [get_embedding_variable("%s/part_%d" % (name, p), embedding_dim, key_dtype,
                                       initializer, steps_to_live, ev_option, capacity, device,
                                       l2_weight_threshold=l2_weight_threshold,
                                       value_dtype=value_dtype)
                for p in range(int(partitioner))]
    if name in _EV_REGISTRY:
        return _EV_REGISTRY[name]
    ev = EmbeddingVariable(name, embedding_dim, initializer, steps_to_live, ev_option, capacity,
                           device, l2_weight_threshold=l2_weight_threshold, key_dtype=key_dtype,
                           value_dtype=value_dtype)
    _EV_REGISTRY[name] = ev
    return ev


def reset_registry():
    _EV_REGISTRY.clear()


# ---------------------------------------------------------------------------
# MultiHashVariable (kv_variable_ops.py:768 MultiHashVariable,
# variable_scope.py get_multihash_variable), "Q-R" strategy
# ---------------------------------------------------------------------------
class MultiHashVariableConfig(object):
    """size = [[Q, Dq], [R, Dr]], strategy "Q-R", operation add / mul / concat."""

    def __init__(self, size, strategy="Q-R", operation="add"):
        if strategy != "Q-R":
            raise ValueError("complementary_strategy %r: only \"Q-R\" is built" % (strategy,))
        if operation not in _lib.MHV_OPERATIONS:
            raise ValueError("operation %r: must be one of 'add', 'mul' or 'concat'"
                             % (operation,))
        try:
            size = [[int(x) for x in pair] for pair in size]
        except (TypeError, ValueError):
            size = None
        if (size is None or len(size) != 2 or any(len(p) != 2 for p in size)
                or any(x < 1 for p in size for x in p)):
            raise ValueError("dims must be [[Q, Dq], [R, Dr]] with rows >= 1 and dim >= 1")
        if operation != "concat" and size[0][1] != size[1][1]:
            raise ValueError("dims: operation %r needs Dq == Dr (got %d and %d)"
                             % (operation, size[0][1], size[1][1]))
        self.size = size
        self.strategy = strategy
        self.operation = operation


class MultiHashVariable(object):
    """Two small dense tables standing for one large one (the quotient-
    remainder trick): id -> Q[id // Q_rows] (op) R[id % R_rows], the divisor
    of the quotient being the Q table's row count (csrc/dr_multihash.h holds
    the rule).  val_list = [Q table, R table] (DenseTables, fp32); the pooled
    and unpooled lookups of embedding_ops combine the two rows inside the
    kernel, and the backward queues IndexedSlices on both tables."""

    def __init__(self, name, val_list, mhvconfig):
        if len(val_list) != 2:
            raise ValueError("val_list must hold the Q and the R table")
        for t, (rows, dim) in zip(val_list, mhvconfig.size):
            if t.weight.dtype != torch.float32:
                raise TypeError("MultiHashVariable %s: tables must be float32 (got %s)"
                                % (name, t.weight.dtype))
            if tuple(t.weight.shape) != (rows, dim):
                raise ValueError("MultiHashVariable %s: table shape %s does not match dims %s"
                                 % (name, tuple(t.weight.shape), [rows, dim]))
        if val_list[0].device != val_list[1].device:
            raise ValueError("MultiHashVariable %s: both tables must be on one device" % name)
        self.name = name
        self._val_list = list(val_list)
        self.mhvconfig = mhvconfig
        self.device = val_list[0].device
        (_, dq), (_, dr) = mhvconfig.size
        self.dim = dq + dr if mhvconfig.operation == "concat" else dq

    @property
    def val_list(self):
        return self._val_list

    @property
    def operation(self):
        return self.mhvconfig.operation

    def get_shape(self):
        """(ids with a valid quotient, dim): the table the variable stands for."""
        q_rows = self.mhvconfig.size[0][0]
        return (q_rows * q_rows, self.dim)


def _mhv_table(name, initializer, rows, dim, device):
    from .embedding_ops import DenseTable
    if initializer is None:
        initializer = 0.0
    if torch.is_tensor(initializer):
        if initializer.dtype != torch.float32:
            raise TypeError("%s: the tables are float32 (initializer is %s)"
                            % (name, initializer.dtype))
        if tuple(initializer.shape) != (rows, dim):
            raise ValueError("%s: initializer shape %s, table shape %s"
                             % (name, tuple(initializer.shape), (rows, dim)))
        w = initializer.detach().clone()
    elif callable(initializer):
        w = torch.as_tensor(initializer((rows, dim)))
        if w.dtype != torch.float32:
            raise TypeError("%s: the tables are float32 (initializer gave %s)" % (name, w.dtype))
        w = w.reshape(rows, dim).clone()
    else:
        w = torch.full((rows, dim), float(initializer), dtype=torch.float32)
    t = DenseTable(w.to(device))
    t.name = name
    return t


def get_multihash_variable(name, dims, complementary_strategy="Q-R", operation="add",
                           initializer=None, device=None):
    """tf.get_multihash_variable (variable_scope.py) without partitioners.

    dims = [[Q, Dq], [R, Dr]].  initializer: a callable given each table's
    shape, a tensor taken as is (both tables of its shape), a scalar, or a pair
    of those (Q's, R's); default as an EmbeddingVariable's default row, 0."""
    cfg = MultiHashVariableConfig(dims, complementary_strategy, operation)
    dev = torch.device(device) if device is not None else \
        torch.device("cuda", torch.cuda.current_device())
    inits = list(initializer) if isinstance(initializer, (list, tuple)) else [initializer] * 2
    if len(inits) != 2:
        raise ValueError("initializer: one value, or a pair (Q's, R's)")
    tables = [_mhv_table("%s/%s" % (name, part), init, rows, dim, dev)
              for part, init, (rows, dim) in zip("QR", inits, cfg.size)]
    return MultiHashVariable(name, tables, cfg)


# ---------------------------------------------------------------------------
# AdaptiveEmbeddingVariable (variable_scope.py get_adaptive_embedding_variable,
# embedding_ops.py adaptive_embedding_lookup_sparse): hot ids in an EV, cold
# ids in a shared hash-bucket table
# ---------------------------------------------------------------------------
def _refuse_adaptive(what):
    raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT,
                                    "an AdaptiveEmbeddingVariable does not take " + what)


class AdaptiveEmbeddingVariable(object):
    """An EmbeddingVariable for the ids a mask names (private, collision-free
    rows) over a small static hash-bucket table that all the other ids share:
    id -> ev[id] where the mask is set, else hash_table[floormod(id,
    bucket_size)] (csrc/dr_adaptive.h holds the rule).  An id that moves into
    the EV starts from the hash row it has been training.  val_list =
    [hash_table (DenseTable, fp32), ev (EmbeddingVariable, fp32)]; the lookups
    of embedding_ops take the mask (adaptive_mask_tensor) and the backward
    queues IndexedSlices on both members."""

    def __init__(self, name, hash_table, ev):
        if ev.value_dtype != torch.float32:
            _refuse_adaptive("a %s EmbeddingVariable (%s): both members are float32"
                             % (ev.value_dtype, ev.name))
        if ev.tiered:
            _refuse_adaptive("an HBM_DRAM EmbeddingVariable (%s): an id the host tier holds "
                             "would be served its hash row" % ev.name)
        if hash_table.weight.dtype != torch.float32:
            _refuse_adaptive("a %s hash table" % (hash_table.weight.dtype,))
        if hash_table.dim != ev.dim:
            raise ValueError("AdaptiveEmbeddingVariable %s: hash table dim %d, EV dim %d"
                             % (name, hash_table.dim, ev.dim))
        if hash_table.device != ev.device:
            raise ValueError("AdaptiveEmbeddingVariable %s: both members must be on one device"
                             % name)
        self.name = name
        self.hash_table = hash_table
        self.ev = ev
        self.dim = ev.dim
        self.device = ev.device
        self.bucket_size = int(hash_table.weight.shape[0])

    @property
    def val_list(self):
        return [self.hash_table, self.ev]

    def get_shape(self):
        return self.ev.get_shape()


def get_adaptive_embedding_variable(name, embedding_dim, bucket_size, initializer=None,
                                    ev_option=None, key_dtype=torch.int64, device=None):
    """tf.get_adaptive_embedding_variable (variable_scope.py) without
    partitioners: the hash table `name/hash` [bucket_size, embedding_dim] (the
    initializer: a callable given the shape, a tensor taken as is, or a
    scalar; default 0) and the EV `name/ev` made by get_embedding_variable with
    ev_option (filters, GlobalStepEvict and init_option as for any EV; its
    keys' initial rows come from the hash table, not from an initializer)."""
    if name in _EV_REGISTRY:
        return _EV_REGISTRY[name]
    bucket_size = int(bucket_size)
    if bucket_size < 1:
        raise ValueError("bucket_size must be >= 1")
    so = getattr(ev_option, "storage_option", None)
    if so is not None and so.storage_type == StorageType.HBM_DRAM:
        _refuse_adaptive("an HBM_DRAM EmbeddingVariable (%s): an id the host tier holds would be "
                         "served its hash row" % name)
    dev = torch.device(device) if device is not None else \
        torch.device("cuda", torch.cuda.current_device())
    table = _mhv_table("%s/hash" % name, initializer, bucket_size, int(embedding_dim), dev)
    ev = get_embedding_variable("%s/ev" % name, embedding_dim, key_dtype=key_dtype,
                                ev_option=ev_option, device=dev)
    var = AdaptiveEmbeddingVariable(name, table, ev)
    _EV_REGISTRY[name] = var
    return var


def refuse_adaptive(evs, what):
    """The sharded engines shard EmbeddingVariables by key; an
    AdaptiveEmbeddingVariable's lookup needs its mask and both its members on
    one device."""
    for ev in evs or ():
        if isinstance(ev, AdaptiveEmbeddingVariable):
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "%s shards EmbeddingVariables; %s is an "
                "AdaptiveEmbeddingVariable (look it up locally with "
                "adaptive_embedding_lookup_sparse)" % (what, ev.name))
