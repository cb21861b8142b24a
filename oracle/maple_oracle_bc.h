/*
 * oracle/maple_oracle_bc.h -- TEST INFRASTRUCTURE ONLY: the branch counters of the coverage gate
 * (tests/test_list_edges_coverage.py; the search's own, at the end, are those of tests/test_search_trees.py).  Included by
 * maple_oracle.c and maple_oracle_search.c only under -DOMO_BRANCH_COUNTS; the default build, the one the golden tests pin, never
 * sees this file.
 *
 * Each counter counts one rarely taken branch of an operator.  OMO_BC_PASS(E, name) makes two counters, E_DOWN and E_UP
 * (= E_DOWN + 1), one per direction of passGenomeListThroughBranch: BC(E_DOWN + dirIsUp).
 */
#ifndef MAPLE_ORACLE_BC_H
#define MAPLE_ORACLE_BC_H

#define OMO_BC_PASS(X, E, name) X(E##_DOWN, "pass_down_" name) X(E##_UP, "pass_up_" name)

#define OMO_BC_LIST(X) \
    X(BC_APPEND_R_D1_O, "append_R_d1_O")                   /* appendProbNode: R with d0 and d1 against an O vector at <= 0.02, M:6611-6633 */ \
    X(BC_APPEND_NUC_D1_O, "append_nuc_d1_O")               /* appendProbNode: nucleotide with d0 and d1 against an O vector at <= 0.02, M:6744-6761 */ \
    X(BC_APPEND_CARRY3, "append_carry3")                   /* appendProbNode: a third carry-over within one call, M:6772-6783 */ \
    X(BC_MERGE_CARRY, "merge_carry")                       /* mergeVectors(returnLK): the running factor carried over into the log, M:4830-4839 */ \
    X(BC_MERGE_UNDERFLOW, "merge_underflow")               /* mergeVectors(returnLK): the running factor below DBL_MIN (the reference raises, M:4831-4836) */ \
    X(BC_MERGE_UPDOWN_N_ERR_D0, "merge_updown_N_err_d0")   /* mergeVectors(isUpDown), error model: N against an entry that carries d0, M:4517-4518 */ \
    X(BC_MERGE_UPDOWN_N_O_ZERO, "merge_updown_N_O_zero")   /* mergeVectors(isUpDown): N against an O vector of total length 0, M:4560-4561 */ \
    X(BC_BLEN_NONE_R_D1, "blen_none_R_d1")                 /* estimateBranchLengthWithDerivative: None, R with d1 against a zero rate, M:5171-5172 */ \
    X(BC_BLEN_NONE_R_FLAG, "blen_none_R_flag")             /* ... None, tail-less R against a flagged nucleotide over a zero rate, M:5178-5179 */ \
    X(BC_BLEN_NONE_NUC_D1, "blen_none_nuc_d1")             /* ... None, nucleotide with d1 against a zero rate, M:5241-5242 */ \
    X(BC_BLEN_EARLY_TENTH, "blen_early_tenth")             /* ... the early return of 0.1 when vDown > c1 + sens and tDown >= 0.1, M:5341-5342 */ \
    X(BC_EVALPLACE_TOP_FALLBACK, "evalplace_top_fallback") /* evaluatePlacement: the top merge returned None, bestTop = defaultBLen * 0.1, M:6798-6802 */ \
    /* shorten, M:3721-3745: an absorb per tuple length; the decisions on which the run's first entry (entryOld, never        \
     * refreshed after a pop) and the neighbour (the entry popped last) disagree; a refusal on the flag alone */              \
    X(BC_SHORTEN_ABSORB_LEN2, "shorten_absorb_len2")                                                                         \
    X(BC_SHORTEN_ABSORB_LEN3, "shorten_absorb_len3")       /* without an error model only */                                 \
    X(BC_SHORTEN_ABSORB_LEN4, "shorten_absorb_len4")                                                                         \
    X(BC_SHORTEN_ABSORB_LEN5, "shorten_absorb_len5")       /* with an error model only */                                    \
    X(BC_SHORTEN_REFUSE_HEAD_FAR, "shorten_refuse_head_far")     /* refused: the neighbour is within thresholdProb, the run's first entry is not */ \
    X(BC_SHORTEN_HEAD_NEAR_NEIGHBOUR_FAR, "shorten_head_near_neighbour_far") /* the neighbour is outside thresholdProb, the run's first entry inside \
                                                                    (the first entry decides: the entry is absorbed, or refused on its flag) */ \
    X(BC_SHORTEN_REFUSE_FLAG, "shorten_refuse_flag")       /* refused on the flag alone: every length within thresholdProb */ \
    /* passGenomeListThroughBranch, M:3749-3877, per direction */                                                           \
    OMO_BC_PASS(X, BC_PASS_MUT_AT_1, "mut_at_1")                                                                             \
    OMO_BC_PASS(X, BC_PASS_MUT_AT_LREF, "mut_at_lRef")                                                                       \
    OMO_BC_PASS(X, BC_PASS_R_MUT_FIRST, "R_mut_first")     /* R run with a mutation on its first site: no stretch before */  \
    OMO_BC_PASS(X, BC_PASS_R_MUT_LAST, "R_mut_last")       /* ... on its last site: no stretch after */                      \
    OMO_BC_PASS(X, BC_PASS_R_MUT_ADJACENT, "R_mut_adjacent") /* ... on two adjacent sites: no stretch between */             \
    OMO_BC_PASS(X, BC_PASS_R_MUT_THREE, "R_mut_three")     /* three or more mutations in one R run */                        \
    OMO_BC_PASS(X, BC_PASS_R_TAIL_LEN3, "R_tail_len3")     /* a mutated R run with a tail, per tuple length (3: plain only; 5: error model only) */ \
    OMO_BC_PASS(X, BC_PASS_R_TAIL_LEN4, "R_tail_len4")                                                                       \
    OMO_BC_PASS(X, BC_PASS_R_TAIL_LEN5, "R_tail_len5")                                                                       \
    OMO_BC_PASS(X, BC_PASS_N_SKIP_ONE, "N_skip_one")       /* an N run that skips one mutation */                            \
    OMO_BC_PASS(X, BC_PASS_N_SKIP_MANY, "N_skip_many")     /* ... several */                                                 \
    OMO_BC_PASS(X, BC_PASS_NUC_TO_R, "nuc_to_R")           /* a nucleotide equal to the new reference becomes R; without a tail */ \
    OMO_BC_PASS(X, BC_PASS_NUC_TO_R_TAIL, "nuc_to_R_tail") /* ... with a tail */                                             \
    OMO_BC_PASS(X, BC_PASS_NUC_KEEPS, "nuc_keeps")         /* a nucleotide that keeps its type with the new reference */     \
    OMO_BC_PASS(X, BC_PASS_O_MUT, "O_mut")                 /* an O entry on a mutated site; without d0 */                    \
    OMO_BC_PASS(X, BC_PASS_O_MUT_D0, "O_mut_d0")           /* ... with d0 */                                                 \
    /* areVectorsDifferent, M:5419-5472: each return of True, and the two passes of unequal O components */                 \
    X(BC_DIFFER_TYPE, "differ_type")                                                                                         \
    X(BC_DIFFER_LEN, "differ_len")                                                                                           \
    X(BC_DIFFER_D0, "differ_d0")                                                                                             \
    X(BC_DIFFER_D1, "differ_d1")                                                                                             \
    X(BC_DIFFER_FLAG4, "differ_flag4")                     /* the flag of a length-4 tuple under an error model */           \
    X(BC_DIFFER_FLAG5, "differ_flag5")                                                                                       \
    X(BC_DIFFER_O_D0, "differ_O_d0")                                                                                         \
    X(BC_DIFFER_O_ZERO, "differ_O_zero")                   /* one of two unequal components is 0 */                          \
    X(BC_DIFFER_O_ABS, "differ_O_abs")                     /* above thresholdDiffForUpdate */                                \
    X(BC_DIFFER_O_FOLD_FIRST, "differ_O_fold_first")       /* fold change by the first quotient only */                      \
    X(BC_DIFFER_O_FOLD_SECOND, "differ_O_fold_second")     /* ... by the second only (both at once cannot be: d / max < 1) */ \
    X(BC_DIFFER_O_SAME_THR, "differ_O_same_thr")           /* unequal, yet the same: difference <= thresholdProb */          \
    X(BC_DIFFER_O_SAME_WINDOW, "differ_O_same_window")     /* ... inside the window with both quotients small */             \
    /* rootVector, M:4916-4996 */                                                                                            \
    X(BC_ROOTVEC_O_ZERO, "rootvec_O_zero")                 /* O with total length 0, no d0 of its own */                     \
    X(BC_ROOTVEC_O_ZERO_D0, "rootvec_O_zero_d0")           /* ... with a d0 (of 0.0) */                                      \
    X(BC_ROOTVEC_O_LEN, "rootvec_O_len")                   /* O with total length != 0, no d0 */                             \
    X(BC_ROOTVEC_O_LEN_D0, "rootvec_O_len_d0")             /* ... with a d0 */                                               \
    X(BC_ROOTVEC_ERR_TAIL, "rootvec_err_tail")             /* error model: the entry has a tail / bLen != 0 or flagged / neither */ \
    X(BC_ROOTVEC_ERR_BLEN, "rootvec_err_blen")                                                                               \
    X(BC_ROOTVEC_ERR_BARE, "rootvec_err_bare")                                                                               \
    X(BC_ROOTVEC_PLAIN_TAIL, "rootvec_plain_tail")         /* no error model: the same three */                              \
    X(BC_ROOTVEC_PLAIN_BLEN, "rootvec_plain_blen")                                                                           \
    X(BC_ROOTVEC_PLAIN_BARE, "rootvec_plain_bare")                                                                           \
    /* findProbRoot, M:4865-4912 */                                                                                          \
    X(BC_ROOTPROB_FLAG_R, "rootprob_flag_R")               /* a flagged R run: the rootFreqsLogErrorCumulative difference */  \
    X(BC_ROOTPROB_FLAG_NUC_GLOBAL, "rootprob_flag_nuc_global") /* a flagged nucleotide under the global error rate */         \
    X(BC_ROOTPROB_FLAG_NUC_SITE, "rootprob_flag_nuc_site") /* ... under site-specific rates */                               \
    X(BC_ROOTPROB_CARRY, "rootprob_carry")                                                                                   \
    X(BC_ROOTPROB_MINUS_INF, "rootprob_minus_inf")                                                                           \
    /* isMinorSequence, M:5918-6003 */                                                                                       \
    X(BC_MINOR_IDENTICAL_TYPE, "minor_identical_type")     /* onlyFindIdentical: two types differ -> 0 */                    \
    X(BC_MINOR_N_R, "minor_N_R")                           /* the ladder: N against R / against a single site, on both sides */ \
    X(BC_MINOR_N_SITE, "minor_N_site")                                                                                       \
    X(BC_MINOR_R_N, "minor_R_N")                                                                                             \
    X(BC_MINOR_SITE_N, "minor_site_N")                                                                                       \
    X(BC_MINOR_O1_BIG, "minor_O1_big")                     /* O on side 1: its component for the other side's nucleotide > 0.1 / not -> 0 */ \
    X(BC_MINOR_O1_SMALL, "minor_O1_small")                                                                                   \
    X(BC_MINOR_O2_BIG, "minor_O2_big")                                                                                       \
    X(BC_MINOR_O2_SMALL, "minor_O2_small")                                                                                   \
    X(BC_MINOR_NUC_MISMATCH, "minor_nuc_mismatch")         /* two different nucleotides (or a nucleotide against R) -> 0 */  \
    X(BC_MINOR_OO_IDENTICAL_DIFF, "minor_OO_identical_diff") /* onlyFindIdentical: two O vectors differ -> 0 */              \
    X(BC_MINOR_OO_IDENTICAL_SAME, "minor_OO_identical_same") /* ... are equal */                                             \
    X(BC_MINOR_OO_FOUND1, "minor_OO_found1")                                                                                 \
    X(BC_MINOR_OO_FOUND2, "minor_OO_found2")                                                                                 \
    X(BC_MINOR_EARLY_BOTH, "minor_early_both")             /* found1bigger and found2bigger -> 0 */                          \
    X(BC_MINOR_END_1_BIGGER, "minor_end_1_bigger")         /* the returns after the loop: 1 (found1bigger), 2, 1 (neither) */ \
    X(BC_MINOR_END_2_BIGGER, "minor_end_2_bigger")                                                                           \
    X(BC_MINOR_END_EQUAL, "minor_end_equal")                                                                                 \
    X(BC_MINOR_END_BOTH, "minor_end_both")                 /* 0 after the loop */

/* The arms of the SPR regraft search (omo_findBestParentTopology, omo_sprWorker), the counters of tests/test_search_trees.py.
 * They follow BC_N in the same array and are read through omo_search_branch_counts, so that omo_branch_counts lists the
 * operators' counters only.  OMO_BC_MERGE(X, E, name) makes two counters for a merge of the search that has no result: E, the
 * reference's "the merge is None" (mergeVectors itself returned None on two lists), and E_ABSENT (= E + 1), an input list the
 * tree does not have. */
#define OMO_BC_MERGE(X, E, name) X(E, "search_" name "_none") X(E##_ABSENT, "search_" name "_absent")

#define OMO_BC_SEARCH_LIST(X) \
    X(BC_SRCH_SEED_ROOT_SIB_INNER, "search_seed_root_sibling_inner") /* the pruned node hangs on the root, its sibling has children, M:6916-6957 */ \
    X(BC_SRCH_SEED_ROOT_SIB_LEAF, "search_seed_root_sibling_leaf")   /* ... its sibling is a leaf: nothing to search */            \
    OMO_BC_MERGE(X, BC_SRCH_DOWN_MID, "down_mid")          /* going down, updating: midTot, M:7037-7044 */                       \
    X(BC_SRCH_DOWN_STOP, "search_down_stop")               /* going down: the stop rule, midTot is the stored probVectTotUp */    \
    X(BC_SRCH_SHORTEN_OWN, "search_shorten_own")           /* M:7087 changes the removed list: the search's own first list */     \
    X(BC_SRCH_SHORTEN_PASSED, "search_shorten_passed")     /* ... a list re-expressed through a reference branch */              \
    OMO_BC_MERGE(X, BC_SRCH_DOWN_VUP, "down_vup")          /* going down, updating: the child's vectUp; the child is not pushed */ \
    OMO_BC_MERGE(X, BC_SRCH_UP_BOTTOM, "up_bottom")        /* crawling up, updating: midBottom, M:7170-7178 */                   \
    X(BC_SRCH_UP_TOTUP_ON_THE_SPOT, "search_up_totup_on_the_spot") /* the node has no probVectTotUp: made on the spot, M:7198-7200 */ \
    OMO_BC_MERGE(X, BC_SRCH_UP_MID, "up_mid")              /* crawling up, updating: midTot */                                   \
    X(BC_SRCH_UP_STOP, "search_up_stop")                   /* crawling up: the stop rule */                                      \
    OMO_BC_MERGE(X, BC_SRCH_UP_VUP, "up_vup")              /* crawling up: the sibling's vectUp (absent: also the cached list) */  \
    OMO_BC_MERGE(X, BC_SRCH_UP_BOTTOM_LATE, "up_bottom_late") /* crawling up: midBottom made late, over a short branch */         \
    X(BC_SRCH_ROOT_CROSS_UPDATING, "search_root_cross_updating")   /* over the root into its other child, rootVector, M:7392-7420 */ \
    X(BC_SRCH_ROOT_CROSS_CACHED, "search_root_cross_cached")                                                                    \
    X(BC_SRCH_SCORE_MINUS_INF, "search_score_minus_inf")   /* a placement scored -inf */                                         \
    X(BC_SRCH_REFINE_NO_LIST, "search_refine_no_list")     /* refinement: a record without up, down or mid list; the reference raises */ \
    OMO_BC_MERGE(X, BC_SRCH_REFINE_LOWER, "refine_lower")  /* refinement: midLower; raises */                                    \
    X(BC_SRCH_REFINE_TOP_RETRY, "search_refine_top_retry") /* refinement: midTop None, retried with top = defaultBLen * 0.1 */    \
    X(BC_SRCH_REFINE_TOP_NONE, "search_refine_top_none")   /* ... None again; raises */                                          \
    X(BC_SRCH_REFINE_NEWMID_NONE, "search_refine_newmid_none") /* refinement: newMid None; raises */                             \
    X(BC_SRCH_STATUS_MINUS_1, "search_status_minus_1")     /* the worker: the search itself raised */                            \
    X(BC_SRCH_STATUS_2, "search_status_2")                 /* the worker: not searched, a zero-length branch with a good cost */   \
    X(BC_SRCH_VETO_PARENT, "search_veto_parent")           /* the accept rule, M:9681-9700: bestNode is the parent */             \
    X(BC_SRCH_CHAIN_STEP, "search_chain_step")             /* ... one step up the chain of zero-length branches */               \
    X(BC_SRCH_VETO_CHAIN_TOP, "search_veto_chain_top")     /* ... bestNode is the chain's top and blen[1] == 0 */                 \
    X(BC_SRCH_VETO_SIBLING, "search_veto_sibling")         /* ... bestNode is the sibling */                                     \
    X(BC_SRCH_VETO_BELOW_SIBLING, "search_veto_below_sibling") /* ... bestNode hangs on the sibling and blen[0] == 0 */

#define OMO_BC_ENUM_(e, n) e,
enum { OMO_BC_LIST(OMO_BC_ENUM_) BC_N, BC_SEARCH_BEFORE_ = BC_N - 1, OMO_BC_SEARCH_LIST(OMO_BC_ENUM_) BC_ALL_N };
extern long long omo_bc[BC_ALL_N];
#define BC(k) __atomic_fetch_add(&omo_bc[k], 1, __ATOMIC_RELAXED)

#endif
