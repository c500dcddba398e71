"""deeprec_amd -- MI355X-native engine for DeepRec's EmbeddingVariable /
embedding_lookup_sparse hot path.

The compute is HIP (gfx950) behind the C ABI in include/deeprec_amd.h; this
package mirrors the reference's Python op surface (tf.get_embedding_variable,
EmbeddingVariable.sparse_read, tf.nn.embedding_lookup_sparse,
safe_embedding_lookup_sparse, fused_embedding_lookup_sparse, the EV sparse
optimizers) on torch device tensors.
"""
from . import _lib
from . import torch_ops  # noqa: F401  (registers torch.ops.deeprec.*)
from ._lib import DeepRecError, InvalidArgumentError, load
from .embedding_ops import (DenseTable, SparseTensor, adaptive_embedding_lookup_sparse,
                            embedding_lookup, embedding_lookup_sparse,
                            embedding_lookup_sparse_multi, fused_embedding_lookup_sparse,
                            safe_embedding_lookup_sparse)
from .kv_variable_ops import (AdaptiveEmbeddingVariable, CBFFilter, CounterFilter,
                              EmbeddingVariable, EmbeddingVariableOption,
                              GlobalStepEvict, IndexedSlices, InitializerOption, KeyBudgetEvict,
                              MultiHashVariable, MultiHashVariableConfig, StorageOption,
                              StorageType, flush_releases, get_adaptive_embedding_variable,
                              get_embedding_variable,
                              get_multihash_variable, read_only_lookups, read_only_serves_tier)
from .ops import gru_sequence, set_validate, status_check
from .string_ops import StringTensor, string_to_hash_bucket_fast
from .training import (AdagradDecayOptimizer, AdagradOptimizer, AdamAsyncOptimizer, AdamOptimizer,
                       FtrlOptimizer, GradientDescentOptimizer)

__all__ = [
    "DeepRecError", "InvalidArgumentError", "load", "DenseTable", "SparseTensor",
    "embedding_lookup", "embedding_lookup_sparse", "embedding_lookup_sparse_multi",
    "fused_embedding_lookup_sparse", "safe_embedding_lookup_sparse", "CBFFilter",
    "CounterFilter", "EmbeddingVariable", "EmbeddingVariableOption", "GlobalStepEvict",
    "IndexedSlices", "KeyBudgetEvict", "get_embedding_variable", "read_only_lookups", "set_validate", "status_check",
    "AdagradOptimizer", "AdagradDecayOptimizer", "AdamAsyncOptimizer", "AdamOptimizer",
    "FtrlOptimizer", "GradientDescentOptimizer", "StringTensor",
    "string_to_hash_bucket_fast", "StorageOption", "StorageType", "InitializerOption",
    "read_only_serves_tier", "MultiHashVariable", "MultiHashVariableConfig",
    "get_multihash_variable", "AdaptiveEmbeddingVariable", "get_adaptive_embedding_variable",
    "adaptive_embedding_lookup_sparse", "gru_sequence",
]
