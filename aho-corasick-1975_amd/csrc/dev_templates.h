/* dev_templates.h -- keyword templates with symbol classes: TEMPLATES of a record set (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * A template is a target of dev_approx.h whose positions are CELLS: a literal cell accepts its spelling's
 * symbol, an ANY cell every symbol, a class cell the symbols of a class.  The pieces stand on literal cells,
 * so seeds, postings, the cheap tests, the passes and the order are APPROX's, and they are APPROX's code: the
 * kernels are approx_count_kernel<T, true> and approx_fill_kernel<T, true> behind offsets_check_kernel, and the
 * three order kernels behind them.  What is new is the acceptance test that a lane of the group runs on its
 * cell, below.  The compiled set (ACMTemplates) adds to APPROX's tables the cell words, one uint32_t beside
 * every symbol of the spellings, and the classes:
 *   1-byte symbols: a bitmap of 256 bits per class, eight 32-bit words, with the negate flag applied at
 *     create; the test is one 32-bit load of word sym >> 5 and a shift.  The bitmaps are read from global
 *     memory: 32 bytes per class, shared by every group, so they stay in cache (DESIGN.md has the measurement).
 *   2-, 4- and 8-byte symbols: the ranges of the class, at most ACM_TEMPLATE_MAX_RANGES pairs lo, hi in the
 *     caller's size, walked in order, and the negate flag from the compiled table.
 * The walk over ranges and the branch on the cell's kind diverge inside a wave, but they hold no cross-lane
 * operation: the round loop around them stays wave-uniform and its __ballot is executed by all 64 lanes.
 * Every address is bounded by what create checked: a class id is below n_classes, and the text index is
 * below the end of the candidate's text. */

/* whether the cell does NOT accept the symbol at text_at; spell_at is the cell's entry of the spelling */
template <typename T>
__device__ __forceinline__ bool
templates_cell_fails (const ApproxK &K, uint32_t cell, const T *__restrict__ text_at, const T *__restrict__ spell_at) {
  if (cell == ACM_TEMPLATE_ANY) /* (no load of the text) */
    return false;
  const T sym = *text_at;
  if (cell == ACM_TEMPLATE_LITERAL)
    return sym != *spell_at;
  if (sizeof (T) == 1)
    return !((K.cls_bitmap[(uint64_t)cell * 8 + ((uint32_t)sym >> 5)] >> ((uint32_t)sym & 31)) & 1);
  const T *__restrict__ ranges = static_cast<const T *> (K.cls_ranges);
  bool in = false;
  for (uint64_t r = K.cls_ptr[cell], end = K.cls_ptr[cell + 1]; r < end && !in; r++)
    in = ranges[2 * r] <= sym && sym <= ranges[2 * r + 1];
  return in == ((K.cls_flags[cell] & ACM_TEMPLATE_NEGATED) != 0);
}
