"""MI355X-native Aho-Corasick scan engine behind the acm_* C API of farhiongit/aho-corasick-1975.

The product is the C-ABI shared library `libac75_amd.so` (host acm_* API in C, flattener in C,
scan kernels in HIP for gfx950; sources under csrc/, headers under /include).  This package is
the thin Python host layer over that C ABI: ctypes bindings that mirror the reference's API
names, plus torch plumbing (device buffers, streams, torch.distributed) for the bulk scan.

There is no CPU scan path here: the bulk scan raises if the library or a GPU is missing.
"""
from .binding import (  # noqa: F401
    ACMError, Machine, Plan, Stream, MultiScan, Comm, FlatTables, RECORD_DTYPE, build_native, lib, library_path,
    select_records, replace_records, replacement_table, Replaced,
    tokens_records, Tokens, TOKENS_GAP_SYMBOL, TOKENS_GAP_RUN, TOKENS_GAP_DROP,
    grep_gather, Grepped, split_offsets,
    tally_batch_records, TalliedBatch,
    rule, present, absent, between, RuleSet, Rules, Fired, rules_matrix, ACM_RULE_NO_MAX,
    weight, score_class, ScoreModel, Score, Scored, ScoreInfo, score_matrix, score_top, ACM_SCORE_NO_CAP, ACM_SCORE_NONE, ACM_SCORE_TOP_MAX,
    Indexed, index_matrix, index_concat,
    words_records, ASCII_WORD, ACM_WORDS_LEFT, ACM_WORDS_RIGHT, ACM_WORDS_BOTH,
    context_records, Snippets, ACM_CONTEXT_SYMBOLS, ACM_CONTEXT_TEXTS, ACM_CONTEXT_EACH, ACM_CONTEXT_MERGE, ACM_CONTEXT_NONE,
    anchored_records, ACM_ANCHORED_PREFIXES, ACM_ANCHORED_LONGEST, ACM_ANCHORED_WHOLE, ACM_LOOKUP_NONE,
    PatternSet, Patterns, patterns_records,
    ApproxSet, Approx, approx_records, edit_records,
    TemplateSet, Templates, SymbolClass, ANY, IUPAC, template, hex_template, templates_records,
    ACM_TEMPLATE_LITERAL, ACM_TEMPLATE_ANY, ACM_TEMPLATE_NEGATED, ACM_TEMPLATE_MAX_RANGES,
    ChainSet, Chains, ChainsInfo, chains_records,
    NearSet, Near, NearInfo, near_records, NEAR_EXPORTS,
    Cooccurred, cooccur_matrix, cooccur_add, COOCCUR_EXPORTS, ACM_COOCCUR_PRODUCT, ACM_COOCCUR_DIAGONAL,
    chars_records, chars_positions, CHARS_EXPORTS, STR_MATCH_DTYPE, ACM_CHARS_CODEPOINTS, ACM_CHARS_UTF16,
    ACM_CHARS_EDGE_START, ACM_CHARS_EDGE_END, ACM_CHARS_EDGE_BAD,
)
from . import synth  # noqa: F401
from . import sharded  # noqa: F401
