/*
 * strelka_oracle.c -- CPU restatement of the Strelka2 hot path.  TEST INFRASTRUCTURE ONLY (see strelka_oracle.h).
 *
 * Every function cites the reference lines it follows (L/ = /root/reference/src/c++/lib/).  Float/double mixing is
 * restated literally (blt_float_t == float, L/blt_util/blt_types.hh:27): where the reference's C++ expression
 * promotes to double (a `1.` or `0.5` literal) the restatement does too.
 *
 * Build: gcc -O2 -std=c11 -ffp-contract=off -fPIC -shared strelka_oracle.c -lm   (no FMA contraction: the reference
 * is built for baseline x86-64, which has none).
 */
#define _GNU_SOURCE
#include "strelka_oracle.h"

#include <assert.h>
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------------------------------------ scalar helpers */

/* L/blt_util/math_util.hh:33-48 (double) */
double sko_log1p_switch(double x)
{
    if (fabs(x) < 0.01) return log1p(x);
    return log(1 + x);
}

/* L/blt_util/math_util.hh:33-48 (float instantiation: smallx_thresh is float(0.01)) */
static float log1p_switch_f(float x)
{
    static const float smallx_thresh = 0.01f;
    if (fabsf(x) < smallx_thresh) return log1pf(x);
    return logf(1 + x);
}

/* L/blt_util/logSumUtil.hh:33-41 */
double sko_log_sum2(double x1, double x2)
{
    if (x1 < x2) { double t = x1; x1 = x2; x2 = t; }
    return x1 + sko_log1p_switch(exp(x2 - x1));
}

float sko_log_sum2f(float x1, float x2)
{
    if (x1 < x2) { float t = x1; x1 = x2; x2 = t; }
    return x1 + log1p_switch_f(expf(x2 - x1));
}

/* L/blt_util/qscore.hh:40-47,60-66 (double) */
int sko_error_prob_to_qphred(double prob)
{
    static const double minlog10 = (double)DBL_MIN_10_EXP;
    const double l = log10(prob);
    const double m = (minlog10 < l) ? l : minlog10; /* std::max(minlog10, l) */
    const double phred = -10. * m;
    return (int)floor(phred + 0.5);
}

/* L/blt_util/qscore.hh:49-57,68-74 (float): ln10 = logf(10), division and max in float, `-10.*` in double, result
 * narrowed to float by the FloatType return, `+0.5` in double. */
int sko_ln_error_prob_to_qphred_f(float lnProb)
{
    static const float minlog10 = (float)FLT_MIN_10_EXP;
    const float ln10 = logf(10.f);
    const float q = lnProb / ln10;
    const float m = (minlog10 < q) ? q : minlog10;
    const float phred = (float)(-10. * m);
    return (int)floor(phred + 0.5);
}

/* ------------------------------------------------------------------------------------------------ q-score tables */

enum { MAX_QSCORE = 70 };
static double g_q2p[MAX_QSCORE + 1], g_q2lncompe[MAX_QSCORE + 1], g_q2lne[MAX_QSCORE + 1];
static int g_tables_ready = 0;

/* L/blt_util/qscore_cache.cpp:34-50 */
static void init_tables(void)
{
    if (g_tables_ready) return;
    const double q2lnp = -log(10.) / 10.;
    for (int i = 0; i <= MAX_QSCORE; ++i) {
        g_q2p[i] = pow(10., -((double)i) / 10.); /* phred_to_error_prob, qscore.hh:77-82 */
        g_q2lncompe[i] = sko_log1p_switch(-g_q2p[i]);
        g_q2lne[i] = (double)i * q2lnp;
    }
    g_tables_ready = 1;
}

void sko_get_qscore_tables(double* q2p, double* q2lncompe, double* q2lne)
{
    init_tables();
    memcpy(q2p, g_q2p, sizeof(g_q2p));
    memcpy(q2lncompe, g_q2lncompe, sizeof(g_q2lncompe));
    memcpy(q2lne, g_q2lne, sizeof(g_q2lne));
}

/* packed base_call accessors (layout: include/strelka_amd.h; L/blt_common/snp_pos_info.hh:109-117) */
#define C_Q(c) ((unsigned)((c) & 0x3f))
#define C_BASE(c) ((unsigned)(((c) >> 6) & 0xf))
#define C_FWD(c) ((unsigned)(((c) >> 10) & 1))
#define C_NMM(c) ((unsigned)(((c) >> 11) & 1))
#define C_FILTER(c) ((unsigned)(((c) >> 12) & 1))

/* ------------------------------------------------------------------------------ libstdc++ std::sort, restated
 * GCC 11 bits/stl_algo.h: __sort = __introsort_loop(first,last,2*lg(n)) + __final_insertion_sort, threshold 16;
 * bits/stl_heap.h for the depth-limit fallback.  comp(a,b) := key[a] > key[b]
 * (sort_icall_by_eprob, L/blt_common/adjust_joint_eprob.cpp:41-53). */

#define SCMP(a, b) (key[(a)] > key[(b)])

static void s_unguarded_linear_insert(uint32_t* last, const uint16_t* key)
{
    uint32_t val = *last;
    uint32_t* next = last - 1;
    while (SCMP(val, *next)) {
        *last = *next;
        last = next;
        --next;
    }
    *last = val;
}

static void s_insertion_sort(uint32_t* first, uint32_t* last, const uint16_t* key)
{
    if (first == last) return;
    for (uint32_t* i = first + 1; i != last; ++i) {
        if (SCMP(*i, *first)) {
            uint32_t val = *i;
            memmove(first + 1, first, (size_t)(i - first) * sizeof(uint32_t));
            *first = val;
        } else {
            s_unguarded_linear_insert(i, key);
        }
    }
}

static void s_push_heap(uint32_t* first, long hole, long top, uint32_t value, const uint16_t* key)
{
    long parent = (hole - 1) / 2;
    while (hole > top && SCMP(first[parent], value)) {
        first[hole] = first[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    first[hole] = value;
}

static void s_adjust_heap(uint32_t* first, long hole, long len, uint32_t value, const uint16_t* key)
{
    const long top = hole;
    long child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (SCMP(first[child], first[child - 1])) child--;
        first[hole] = first[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        first[hole] = first[child - 1];
        hole = child - 1;
    }
    s_push_heap(first, hole, top, value, key);
}

/* how often the depth-limit fallback ran (a test counter: tests that mean to drive the heap sort ask whether they did) */
static unsigned long g_heap_sort_runs;
unsigned long sko_heap_sort_runs(void) { return g_heap_sort_runs; }
void sko_heap_sort_runs_reset(void) { g_heap_sort_runs = 0; }

static void s_heap_sort(uint32_t* first, uint32_t* last, const uint16_t* key)
{
    ++g_heap_sort_runs;
    /* __partial_sort(first,last,last) = __heap_select (make_heap only, as middle==last) + __sort_heap */
    const long len = last - first;
    if (len >= 2) {
        long parent = (len - 2) / 2;
        for (;;) {
            uint32_t value = first[parent];
            s_adjust_heap(first, parent, len, value, key);
            if (parent == 0) break;
            parent--;
        }
    }
    while (last - first > 1) {
        --last;
        uint32_t value = *last;
        *last = *first;
        s_adjust_heap(first, 0, last - first, value, key);
    }
}

static void s_move_median_to_first(uint32_t* result, uint32_t* a, uint32_t* b, uint32_t* c, const uint16_t* key)
{
    uint32_t* pick;
    if (SCMP(*a, *b)) {
        if (SCMP(*b, *c)) pick = b;
        else if (SCMP(*a, *c)) pick = c;
        else pick = a;
    } else if (SCMP(*a, *c)) pick = a;
    else if (SCMP(*b, *c)) pick = c;
    else pick = b;
    uint32_t t = *result; *result = *pick; *pick = t;
}

static uint32_t* s_unguarded_partition(uint32_t* first, uint32_t* last, uint32_t* pivot, const uint16_t* key)
{
    for (;;) {
        while (SCMP(*first, *pivot)) ++first;
        --last;
        while (SCMP(*pivot, *last)) --last;
        if (!(first < last)) return first;
        uint32_t t = *first; *first = *last; *last = t;
        ++first;
    }
}

static void s_introsort_loop(uint32_t* first, uint32_t* last, long depth_limit, const uint16_t* key)
{
    while (last - first > 16) {
        if (depth_limit == 0) {
            s_heap_sort(first, last, key);
            return;
        }
        --depth_limit;
        uint32_t* mid = first + (last - first) / 2;
        s_move_median_to_first(first, first + 1, mid, last - 1, key);
        uint32_t* cut = s_unguarded_partition(first + 1, last, first, key);
        s_introsort_loop(cut, last, depth_limit, key);
        last = cut;
    }
}

void sko_sort_idx_by_key_desc(uint32_t* idx, int n, const uint16_t* key)
{
    if (n <= 0) return;
    long lg = 0;
    for (unsigned long m = (unsigned long)n; m > 1; m >>= 1) ++lg; /* std::__lg */
    s_introsort_loop(idx, idx + n, lg * 2, key);
    if (n > 16) {
        s_insertion_sort(idx, idx + 16, key);
        for (uint32_t* i = idx + 16; i != idx + n; ++i) s_unguarded_linear_insert(i, key);
    } else {
        s_insertion_sort(idx, idx + n, key);
    }
}

/* ------------------------------------------------------------------------------------------------ hot path A */

static int is_align_match(uint32_t t) { return t == SKO_MATCH || t == SKO_SEQ_MATCH || t == SKO_SEQ_MISMATCH; }
static int is_type_indel(uint32_t t) { return t == SKO_INSERT || t == SKO_DELETE; }

/* L/blt_util/align_path.cpp:868-895 */
static int is_segment_swap_start(const sko_path_seg* path, int n, int i)
{
    int is_insert = 0, is_delete = 0;
    for (; i < n; ++i) {
        if (path[i].type == SKO_INSERT) is_insert = 1;
        else if (path[i].type == SKO_DELETE) is_delete = 1;
        else break;
    }
    return is_insert && is_delete;
}

/* L/htsapi/bam_seq.hh:73-92 */
static uint8_t bam_code_of_char(char c)
{
    switch (c) {
    case '=': return 0;
    case 'A': return 1;
    case 'C': return 2;
    case 'G': return 4;
    case 'T': return 8;
    default: return 15;
    }
}

typedef struct seq_view {
    const char* s;
    int32_t offset; /* genomic position of s[0] (0 for insert sequences) */
    int32_t len;
} seq_view;

/* string_bam_seq / rc_segment_bam_seq ::get_code (L/htsapi/bam_seq.hh:250-300,
 * L/blt_util/reference_contig_segment.hh:46-51): out of range -> 'N' */
static uint8_t seq_code(const seq_view* v, int32_t pos)
{
    if (pos < v->offset || pos >= v->offset + v->len) return 15;
    return bam_code_of_char(v->s[pos - v->offset]);
}

/* scoreMatchSegment / scoreInsertSegment (L/starling_common/starling_read_align_score.cpp:110-170; identical bodies) */
static void score_segment(unsigned seg_length, const uint8_t* read_code, int32_t read_len, const uint8_t* qual,
                          unsigned read_offset, const seq_view* ref, int32_t ref_head_pos, double* lnp)
{
    const double lnthird = -log(3.);
    for (unsigned i = 0; i < seg_length; ++i) {
        const int32_t readPos = (int32_t)(read_offset + i);
        const uint8_t sbase = (readPos >= 0 && readPos < read_len) ? read_code[readPos] : 15; /* bam_seq::get_code */
        if (sbase == 15) continue;
        const uint8_t qscore = qual[readPos];
        int is_ref = (sbase == 0);
        if (!is_ref) {
            const int32_t refPos = ref_head_pos + (int32_t)i;
            is_ref = (sbase == seq_code(ref, refPos));
        }
        *lnp += (is_ref ? g_q2lncompe[qscore] : g_q2lne[qscore] + lnthird);
    }
}

/* getMatchingIndelKey (L/starling_common/starling_read_align_score.cpp:177-228) */
static const sko_indel* get_matching_indel(const sko_cal* cal, int32_t ref_head_pos, unsigned delete_length,
                                           unsigned insert_length, int ends_first, int ends_second, int path_index)
{
    if (path_index < ends_first) return &cal->leading;
    if (path_index > ends_second) return &cal->trailing;
    const sko_indel* found = NULL;
    for (int k = 0; k < cal->n_indels; ++k) {
        const sko_indel* ci = &cal->indels[k];
        if (ci->pos == ref_head_pos && (ci->type == SKO_INDEL_INDEL || ci->type == SKO_INDEL_MISMATCH) &&
            ci->del_len == delete_length && ci->ins_len == insert_length) {
            assert(found == NULL);
            found = ci;
        } else if (ci->pos > ref_head_pos) {
            break;
        }
    }
    assert(found != NULL);
    return found;
}

/* scoreCandidateAlignment (L/starling_common/starling_read_align_score.cpp:261-499) */
double sko_score_candidate_alignment(const uint8_t* read_code, const uint8_t* read_qual, int32_t read_len,
                                     const sko_cal* cal, const char* ref_seq, int32_t ref_offset, int32_t ref_len)
{
    init_tables();
    double lnp = 0.;
    const seq_view ref = { ref_seq, ref_offset, ref_len };
    const sko_path_seg* path = cal->path;
    const int aps = cal->n_seg;

    unsigned read_offset = 0;
    int32_t ref_head_pos = cal->pos;

    /* get_match_edge_segments (L/blt_util/align_path.cpp:735-752) */
    int ends_first = aps, ends_second = aps;
    {
        int is_first_match = 0;
        for (int i = 0; i < aps; ++i) {
            if (is_align_match(path[i].type)) {
                if (!is_first_match) ends_first = i;
                is_first_match = 1;
                ends_second = i;
            }
        }
    }

    int path_index = 0;
    while (path_index < aps) {
        const int is_swap_start = is_segment_swap_start(path, aps, path_index);
        unsigned n_seg = 1;
        const sko_path_seg* ps = &path[path_index];
        const sko_indel* indelKey = NULL;

        if (is_swap_start || ps->type == SKO_SEQ_MISMATCH) {
            unsigned deleteLength, insertLength;
            if (ps->type == SKO_SEQ_MISMATCH) {
                deleteLength = ps->length;
                insertLength = ps->length;
            } else {
                /* swap_info (L/blt_util/align_path_util.hh:75-106) */
                int k = path_index;
                insertLength = 0;
                deleteLength = 0;
                for (; k < aps && is_type_indel(path[k].type); ++k) {
                    if (path[k].type == SKO_INSERT) insertLength += path[k].length;
                    else deleteLength += path[k].length;
                }
                n_seg = (unsigned)(k - path_index);
            }
            indelKey = get_matching_indel(cal, ref_head_pos, deleteLength, insertLength, ends_first, ends_second,
                                          path_index);
            const seq_view ins = { indelKey->ins_seq, 0, (int32_t)indelKey->ins_len };
            int32_t insert_seq_head_pos = 0;
            if (path_index < ends_first) insert_seq_head_pos = (int32_t)ins.len - (int32_t)ps->length;
            score_segment(insertLength, read_code, read_len, read_qual, read_offset, &ins, insert_seq_head_pos, &lnp);
        } else if (is_align_match(ps->type)) {
            score_segment(ps->length, read_code, read_len, read_qual, read_offset, &ref, ref_head_pos, &lnp);
        } else if (ps->type == SKO_INSERT) {
            indelKey = get_matching_indel(cal, ref_head_pos, 0, ps->length, ends_first, ends_second, path_index);
            const seq_view ins = { indelKey->ins_seq, 0, (int32_t)indelKey->ins_len };
            int32_t insert_seq_head_pos = 0;
            if (path_index < ends_first) insert_seq_head_pos = (int32_t)ins.len - (int32_t)ps->length;
            score_segment(ps->length, read_code, read_len, read_qual, read_offset, &ins, insert_seq_head_pos, &lnp);
        } else if (ps->type == SKO_DELETE || ps->type == SKO_SKIP) {
            if (ps->type == SKO_DELETE)
                indelKey = get_matching_indel(cal, ref_head_pos, ps->length, 0, ends_first, ends_second, path_index);
        } else if (ps->type == SKO_SOFT_CLIP) {
            const double unalignedBasecallLogLikelihood = log(0.25);
            lnp += (ps->length * unalignedBasecallLogLikelihood);
        } else if (ps->type == SKO_HARD_CLIP) {
            /* nothing */
        } else {
            assert(0 && "Can't handle cigar code");
        }

        if (indelKey != NULL && indelKey->type != SKO_INDEL_NONE) {
            if (!indelKey->is_candidate) {
                const double nonCandidateIndelPenalty = log(1e-5);
                lnp += nonCandidateIndelPenalty;
            }
        }

        /* increment_path (L/blt_util/align_path_util.hh:38-68) */
        for (unsigned i = 0; i < n_seg; ++i) {
            const sko_path_seg* s = &path[path_index];
            if (is_align_match(s->type)) {
                read_offset += s->length;
                ref_head_pos += (int32_t)s->length;
            } else if (s->type == SKO_DELETE || s->type == SKO_SKIP) {
                ref_head_pos += (int32_t)s->length;
            } else if (s->type == SKO_INSERT || s->type == SKO_SOFT_CLIP) {
                read_offset += s->length;
            }
            path_index++;
        }
    }
    return lnp;
}

/* ------------------------------------------------------------------------------------ hot path B: dependent eprob */

/* get_dependent_eprob (L/blt_common/adjust_joint_eprob.cpp:58-69); all blt_float_t, std::pow(float,float)=powf */
static float dependent_eprob_of(float eprob, float vexp)
{
    static const float dep_converge_prob = 0.75f;
    const float val = powf(eprob, vexp);
    const float frac = (1 - val) / (1 - eprob);
    const float dep = frac * val + (1 - frac) * dep_converge_prob;
    return (eprob < dep) ? dep : eprob; /* std::max(eprob, dep) */
}
static float get_dependent_eprob(unsigned qscore, float vexp)
{
    return dependent_eprob_of((float)g_q2p[qscore], vexp);
}

/* The host libm (and the scalar restatements above) over arrays: see strelka_oracle.h.  Arguments are read through volatile
 * pointers, so that every element is one genuine call of the C library's routine. */
int sko_libm_eval(int fn, int64_t n, const void* a, const void* b, void* out)
{
    const volatile float* af = (const volatile float*)a;
    const volatile float* bf = (const volatile float*)b;
    const volatile double* ad = (const volatile double*)a;
    const volatile double* bd = (const volatile double*)b;
    float* of = (float*)out;
    double* od = (double*)out;
    int32_t* oi = (int32_t*)out;
    for (int64_t i = 0; i < n; ++i) {
        switch (fn) {
        case 0: case 12: of[i] = logf(af[i]); break;
        case 1: of[i] = powf(af[i], bf[i]); break;
        case 2: of[i] = expf(af[i]); break;
        case 3: of[i] = log1pf(af[i]); break;
        case 4: case 8: od[i] = exp(ad[i]); break;
        case 5: case 9: od[i] = log(ad[i]); break;
        case 6: case 10: od[i] = log10(ad[i]); break;
        case 7: case 11: od[i] = log1p(ad[i]); break;
        case 13: of[i] = dependent_eprob_of(af[i], bf[i]); break;
        case 14: oi[i] = sko_ln_error_prob_to_qphred_f(af[i]); break;
        case 15: oi[i] = sko_error_prob_to_qphred(ad[i]); break;
        case 16: od[i] = sko_log1p_switch(ad[i]); break;
        case 17: od[i] = sko_log_sum2(ad[i], bd[i]); break;
        case 18: of[i] = sko_log_sum2f(af[i], bf[i]); break;
        default: return 1;
        }
    }
    return 0;
}

/* adjust_icalls_eprob (L/blt_common/adjust_joint_eprob.cpp:92-194).  `dpc` (dependent_prob_cache) is only ever filled at
 * vexp == min_vexp (is_min_vexp becomes true exactly when vexp is clamped to min_vexp, :170-174), so the cache is the
 * pure function get_dependent_eprob(q, (float)min_vexp). */
static void adjust_icalls_eprob(const sko_germline_options* opt, uint32_t* ic, int ic_size, const uint16_t* calls,
                                const uint16_t* qkey, float* de)
{
    float vexp_frac;
    {
        const float lnran = (float)log(0.75);
        float num = 0, den = 0;
        for (int i = 0; i < ic_size; ++i) {
            const uint16_t bi = calls[ic[i]];
            const float weight = (float)(lnran - g_q2lne[C_Q(bi)]); /* float - double -> double -> float */
            den += weight;
            if (C_NMM(bi)) num += weight;
        }
        float mismatch_frac = 0;
        if (ic_size && (den > 0.)) mismatch_frac = (num / den);
        vexp_frac = (float)((1 - mismatch_frac) * opt->bsnp_ssd_no_mismatch + mismatch_frac * opt->bsnp_ssd_one_mismatch);
    }
    const int is_limit_vexp = opt->is_min_vexp;
    const float min_vexp = (float)opt->min_vexp;
    int is_min_vexp = 0;

    sko_sort_idx_by_key_desc(ic, ic_size, qkey);
    float vexp = 1.f;
    for (int i = 0; i < ic_size; ++i) {
        const uint16_t bi = calls[ic[i]];
        if (!is_min_vexp) {
            de[ic[i]] = get_dependent_eprob(C_Q(bi), vexp);
            float next_vexp = vexp;
            next_vexp *= (1 - vexp_frac);
            if (is_limit_vexp) {
                is_min_vexp = (next_vexp <= min_vexp);
                vexp = (min_vexp < next_vexp) ? next_vexp : min_vexp; /* std::max(min_vexp,next_vexp) */
            } else {
                vexp = next_vexp;
            }
        } else {
            de[ic[i]] = get_dependent_eprob(C_Q(bi), vexp);
        }
    }
}

/* adjust_joint_eprob (L/blt_common/adjust_joint_eprob.cpp:201-243); is_dependent_eprob() assumed true when either
 * ssd parameter > 0 (L/blt_common/blt_shared.hh:75-80, germline: is_bsnp_diploid) */
void sko_adjust_joint_eprob(const uint16_t* calls, int32_t n_calls, const sko_germline_options* opt, float* de)
{
    init_tables();
    for (int i = 0; i < n_calls; ++i) de[i] = (float)g_q2p[C_Q(calls[i])];
    if (!(opt->bsnp_ssd_no_mismatch > 0. || opt->bsnp_ssd_one_mismatch > 0)) return;
    if (n_calls == 0) return;

    uint32_t* ic = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)n_calls);
    uint16_t* qkey = (uint16_t*)malloc(sizeof(uint16_t) * (size_t)n_calls);
    for (int i = 0; i < n_calls; ++i) qkey[i] = (uint16_t)C_Q(calls[i]);
    for (unsigned g = 0; g < 8; ++g) {
        int n = 0;
        for (int i = 0; i < n_calls; ++i) {
            const uint16_t b = calls[i];
            if (C_FILTER(b)) continue;
            if (C_Q(b) < 3) continue;
            const unsigned group_index = C_FWD(b) + 2 * C_BASE(b);
            if (group_index == g) ic[n++] = (uint32_t)i;
        }
        adjust_icalls_eprob(opt, ic, n, calls, qkey, de);
    }
    free(ic);
    free(qkey);
}

/* ------------------------------------------------------------------------------------ hot path B: germline lhood */

/* DIGT::expect2 (L/blt_util/digt.hh:126-146) */
static const uint8_t DIGT_EXPECT2[10][4] = { { 2, 0, 0, 0 }, { 0, 2, 0, 0 }, { 0, 0, 2, 0 }, { 0, 0, 0, 2 }, { 1, 1, 0, 0 },
                                             { 1, 0, 1, 0 }, { 1, 0, 0, 1 }, { 0, 1, 1, 0 }, { 0, 1, 0, 1 }, { 0, 0, 1, 1 } };
/* DIGT::expect (L/blt_util/digt.hh:100-120) as 2*frequency */
#define DIGT_IS_HET(gt) ((gt) >= 4)

/* get_diploid_gt_lhood (L/blt_common/position_snp_call_pprob_digt.cpp:328-385), useHetVariantFrequencyExtension=false */
void sko_diploid_gt_lhood(const uint16_t* calls, const float* de, int32_t n_calls, uint32_t ref_gt,
                          int is_strand_specific, int is_ss_fwd, float* lhood)
{
    init_tables();
    const float one_third = (float)(1. / 3.);
    const float log_one_third = logf(one_third);
    const float one_half = (float)(1. / 2.);
    const float log_one_half = logf(one_half);

    for (unsigned gt = 0; gt < 10; ++gt) lhood[gt] = 0.f;
    for (int i = 0; i < n_calls; ++i) {
        const uint16_t bc = calls[i];
        const float eprob = de[i];
        const float ceprob = (float)(1. - g_q2p[C_Q(bc)]);
        const float lnce = (float)g_q2lncompe[C_Q(bc)];
        float val[3];
        val[0] = logf(eprob) + log_one_third;
        val[1] = (float)(log((ceprob) + ((1. - ceprob) * one_third)) + log_one_half);
        val[2] = lnce;
        const int is_force_ref = (is_strand_specific && (is_ss_fwd != (int)C_FWD(bc)));
        const unsigned obs_id = C_BASE(bc);
        for (unsigned gt = 0; gt < 10; ++gt) lhood[gt] += val[DIGT_EXPECT2[is_force_ref ? ref_gt : gt][obs_id]];
    }
}

typedef struct prior_set {
    float genome[10], poly[10];
} prior_set;

/* priors (L/blt_common/position_snp_call_pprob_digt.cpp:50-258) */
static void build_priors(float theta, prior_set lnprior[5], prior_set lnprior_haploid[5])
{
    const float one_third = (float)(1. / 3.);
    memset(lnprior, 0, sizeof(prior_set) * 5);
    memset(lnprior_haploid, 0, sizeof(prior_set) * 5);
    for (unsigned ref_gt = 0; ref_gt < 4; ++ref_gt) {
        { /* get_genomic_prior :50-74 */
            float* prior = lnprior[ref_gt].genome;
            float prior_sum = 0.f;
            for (unsigned gt = 0; gt < 10; ++gt) {
                if (gt == ref_gt) continue;
                prior[gt] = (theta * one_third);
                if (DIGT_IS_HET(gt)) {
                    if (DIGT_EXPECT2[gt][ref_gt] == 0) prior[gt] *= theta;
                } else {
                    prior[gt] = (float)(prior[gt] * .5);
                }
                prior_sum += prior[gt];
            }
            prior[ref_gt] = (float)(1. - prior_sum);
        }
        { /* get_poly_prior :105-138 */
            float* prior = lnprior[ref_gt].poly;
            const float ctheta = (float)(1. - theta);
            for (unsigned gt = 0; gt < 10; ++gt) {
                if (gt == ref_gt) prior[gt] = (float)(0.25 * (ctheta));
                else if (DIGT_IS_HET(gt)) {
                    if (DIGT_EXPECT2[gt][ref_gt] == 0) prior[gt] = theta * one_third;
                    else prior[gt] = (float)(0.5 * one_third * ctheta);
                } else prior[gt] = (float)(0.25 * one_third * ctheta);
            }
        }
        { /* get_haploid_genomic_prior :78-101 */
            float* prior = lnprior_haploid[ref_gt].genome;
            float prior_sum = 0.f;
            for (unsigned gt = 0; gt < 10; ++gt) {
                if (gt == ref_gt) continue;
                if (DIGT_IS_HET(gt)) prior[gt] = 0;
                else prior[gt] = (theta * one_third);
                prior_sum += prior[gt];
            }
            prior[ref_gt] = (float)(1. - prior_sum);
        }
        { /* get_haploid_poly_prior :142-167 */
            float* prior = lnprior_haploid[ref_gt].poly;
            for (unsigned gt = 0; gt < 10; ++gt) {
                if (gt == ref_gt) prior[gt] = 0.5f;
                else if (DIGT_IS_HET(gt)) prior[gt] = 0;
                else prior[gt] = (float)(0.5 * one_third);
            }
        }
    }
    /* finish_prior :214-237 */
    for (int h = 0; h < 2; ++h) {
        prior_set* P = h ? lnprior_haploid : lnprior;
        for (unsigned i = 0; i < 4; ++i)
            for (unsigned gt = 0; gt < 10; ++gt) {
                P[4].genome[gt] += P[i].genome[gt];
                P[4].poly[gt] += P[i].poly[gt];
            }
        for (int w = 0; w < 2; ++w) { /* norm_gt :184-198 */
            float* x = w ? P[4].poly : P[4].genome;
            float sum = 0;
            for (unsigned gt = 0; gt < 10; ++gt) sum += x[gt];
            sum = (float)(1. / sum);
            for (unsigned gt = 0; gt < 10; ++gt) x[gt] *= sum;
        }
        for (unsigned i = 0; i < 5; ++i)
            for (unsigned gt = 0; gt < 10; ++gt) {
                P[i].genome[gt] = logf(P[i].genome[gt]);
                P[i].poly[gt] = logf(P[i].poly[gt]);
            }
    }
}

void sko_germline_lnpriors(double theta, float* out /* [2][5][2][10]: haploid?, ref, genome/poly, gt */)
{
    prior_set a[5], b[5];
    build_priors((float)theta, a, b);
    for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 5; ++r) {
            const prior_set* p = h ? &b[r] : &a[r];
            memcpy(out + ((h * 5 + r) * 2 + 0) * 10, p->genome, sizeof(float) * 10);
            memcpy(out + ((h * 5 + r) * 2 + 1) * 10, p->poly, sizeof(float) * 10);
        }
}

/* calculate_result_set (L/blt_common/position_snp_call_pprob_digt.cpp:412-433) with normalizeLogDistro and prob_comp
 * (L/blt_util/prob_util.hh:177-237) */
static void calculate_result_set(const float* lhood, const float* lnprior, unsigned ref_gt, sko_digt_result_set* rs)
{
    double pprob[10];
    for (unsigned gt = 0; gt < 10; ++gt) pprob[gt] = lhood[gt] + lnprior[gt]; /* float add, widened */
    unsigned max_idx = 0;
    double max = pprob[0];
    for (unsigned i = 1; i < 10; ++i)
        if (pprob[i] > max) { max = pprob[i]; max_idx = i; }
    double sum = 0.;
    for (unsigned i = 0; i < 10; ++i) { pprob[i] = exp(pprob[i] - max); sum += pprob[i]; }
    sum = 1. / sum;
    for (unsigned i = 0; i < 10; ++i) pprob[i] *= sum;
    rs->max_gt = max_idx;
    rs->ref_pprob = pprob[ref_gt];
    rs->snp_qphred = sko_error_prob_to_qphred(pprob[ref_gt]);
    double comp = 0.;
    for (unsigned i = 0; i < 10; ++i) { if (i == max_idx) continue; comp = comp + pprob[i]; }
    rs->max_gt_qphred = sko_error_prob_to_qphred(comp);
    rs->_pad = 0;
}

/* position_snp_call_pprob_digt (L/blt_common/position_snp_call_pprob_digt.cpp:471-539), is_always_test=true,
 * hetVariantFrequencyExtension=0 */
void sko_position_snp_call_pprob_digt(const uint16_t* calls, const float* de, int32_t n_calls, uint32_t ref_base_id,
                                      int ploidy, const sko_germline_options* opt, sko_digt_call* out)
{
    static prior_set lnprior[5], lnprior_haploid[5];
    static double cached_theta = -1;
    if (cached_theta != opt->bsnp_diploid_theta) {
        build_priors((float)opt->bsnp_diploid_theta, lnprior, lnprior_haploid);
        cached_theta = opt->bsnp_diploid_theta;
    }
    memset(out, 0, sizeof(*out));
    if (ref_base_id >= 4) return; /* 'N' :481 */
    out->is_called = 1;
    out->ref_gt = ref_base_id;
    const int is_haploid = (ploidy == 1);

    float* lhood = out->lhood;
    sko_diploid_gt_lhood(calls, de, n_calls, ref_base_id, 0, 0, lhood);
    {
        unsigned gtcount = 10;
        if (is_haploid) gtcount = 4;
        unsigned maxIndex = 0;
        for (unsigned gt = 1; gt < gtcount; ++gt)
            if (lhood[gt] > lhood[maxIndex]) maxIndex = gt;
        for (unsigned gt = 0; gt < gtcount; ++gt)
            out->phredLoghood[gt] = (uint32_t)sko_ln_error_prob_to_qphred_f(lhood[gt] - lhood[maxIndex]);
    }
    const prior_set* P = is_haploid ? lnprior_haploid : lnprior;
    calculate_result_set(lhood, P[ref_base_id].genome, ref_base_id, &out->genome);
    calculate_result_set(lhood, P[ref_base_id].poly, ref_base_id, &out->poly);

    if (out->genome.snp_qphred != 0) {
        float lhood_fwd[10], lhood_rev[10];
        sko_diploid_gt_lhood(calls, de, n_calls, ref_base_id, 1, 1, lhood_fwd);
        sko_diploid_gt_lhood(calls, de, n_calls, ref_base_id, 1, 0, lhood_rev);
        const unsigned tgt = out->genome.max_gt;
        const float m = (lhood_fwd[tgt] < lhood_rev[tgt]) ? lhood_rev[tgt] : lhood_fwd[tgt];
        out->strand_bias = m - lhood[tgt]; /* float subtraction, widened */
    } else {
        out->strand_bias = 0;
    }
}

/* ------------------------------------------------------------------------------------ hot path B: somatic SNV */

enum { SOM_REF = 0, SOM_HOM = 1, SOM_HET = 2, SOM_SIZE = 3, HET_RES = 9, PRESTRAND = 21, GRID = 30 };

/* DIGT_GRID::get_fraction_from_index (L/applications/strelka/strelka_digt_states.cpp:33-41) */
static float get_fraction_from_index(int index)
{
    const float RATIO_INCREMENT = 0.5f / (float)(HET_RES + 1);
    if (index == SOM_REF) return 0.f;
    if (index == SOM_HOM) return 1.f;
    if (index == SOM_HET) return 0.5f;
    if (index < SOM_SIZE + HET_RES) return RATIO_INCREMENT * (index - SOM_SIZE + 1);
    return RATIO_INCREMENT * (index - SOM_SIZE + 2);
}

void sko_somatic_sample_lhood(const uint16_t* calls, int32_t n_calls, uint32_t ref_gt, int with_strand, float* lhood)
{
    init_tables();
    const float one_third = (float)(1. / 3.);
    const float ln_one_third = logf(one_third);
    const float one_half = (float)(1. / 2.);
    const float ln_one_half = logf(one_half);
    const float RATIO_INCREMENT = 0.5f / (float)(HET_RES + 1);

    for (int i = 0; i < GRID; ++i) lhood[i] = 0.f;

    /* get_diploid_gt_lhood_cached_simple (…_lhood_cached.cpp:41-84) */
    for (int i = 0; i < n_calls; ++i) {
        const uint16_t bc = calls[i];
        const unsigned q = C_Q(bc);
        const float eprob = (float)g_q2p[q];
        const float ceprob = (1 - eprob);
        const float lne = (float)g_q2lne[q];
        const float lnce = (float)g_q2lncompe[q];
        const float v0 = lne + ln_one_third;
        const float v1 = logf((ceprob) + ((eprob)*one_third)) + ln_one_half;
        const float v2 = lnce;
        if (C_BASE(bc) == ref_gt) {
            lhood[SOM_REF] += v2;
            lhood[SOM_HET] += v1;
            lhood[SOM_HOM] += v0;
        } else {
            lhood[SOM_REF] += v0;
            lhood[SOM_HET] += v1;
            lhood[SOM_HOM] += v2;
        }
    }

    /* get_diploid_het_grid_lhood_cached (:133-153) + get_high_low_het_ratio_lhood_cached (:86-131) */
    float* grid = lhood + SOM_SIZE;
    const unsigned totalHetRatios = HET_RES * 2;
    for (unsigned hetIndex = 0; hetIndex < HET_RES; ++hetIndex) {
        const float het_ratio = (hetIndex + 1) * RATIO_INCREMENT;
        const float chet_ratio = (float)(1. - het_ratio);
        float* lhood_high = grid + (totalHetRatios - (hetIndex + 1));
        float* lhood_low = grid + hetIndex;
        for (int i = 0; i < n_calls; ++i) {
            const uint16_t bc = calls[i];
            const float eprob = (float)g_q2p[C_Q(bc)];
            const float ceprob = (1 - eprob);
            const float c0 = logf((ceprob)*het_ratio + ((eprob)*one_third) * chet_ratio);
            const float c1 = logf((ceprob)*chet_ratio + ((eprob)*one_third) * het_ratio);
            if (C_BASE(bc) == ref_gt) {
                *lhood_high += c0;
                *lhood_low += c1;
            } else {
                *lhood_high += c1;
                *lhood_low += c0;
            }
        }
    }

    if (!with_strand) return;
    /* get_diploid_strand_grid_lhood_spi (position_somatic_snv_strand_grid.cpp:63-83) +
     * get_strand_ratio_lhood_spi (…_lhood_cached.cpp:164-234) */
    for (unsigned r = 0; r < HET_RES; ++r) {
        const float het_ratio = (r + 1) * RATIO_INCREMENT;
        const float chet_ratio = (float)(1. - het_ratio);
        float lhood_fwd = 0, lhood_rev = 0;
        for (int i = 0; i < n_calls; ++i) {
            const uint16_t bc = calls[i];
            const unsigned q = C_Q(bc);
            const float eprob = (float)g_q2p[q];
            const float ceprob = (float)(1. - eprob);
            const float c0 = (logf((ceprob)*chet_ratio + ((eprob)*one_third) * het_ratio));
            const float c1 = (logf((ceprob)*het_ratio + ((eprob)*one_third) * chet_ratio));
            if (C_BASE(bc) == ref_gt) {
                const float val_off_strand = (float)g_q2lncompe[q];
                lhood_fwd += (C_FWD(bc) ? c0 : val_off_strand);
                lhood_rev += (C_FWD(bc) ? val_off_strand : c0);
            } else {
                const float val_off_strand = (float)(g_q2lne[q] + ln_one_third);
                lhood_fwd += (C_FWD(bc) ? c1 : val_off_strand);
                lhood_rev += (C_FWD(bc) ? val_off_strand : c1);
            }
        }
        lhood[PRESTRAND + r] = sko_log_sum2f(lhood_fwd, lhood_rev) + ln_one_half;
    }
}

/* calculate_result_set_grid (L/applications/strelka/qscore_calculator.cpp:47-209) */
void sko_calculate_result_set_grid(float contam_tolerance, float logSharedErrorRate, float logSharedErrorRateComplement,
                                   const float* normal_lhood, const float* tumor_lhood,
                                   const float* germlineGenotypeLogPrior, float lnmatch, float lnmismatch,
                                   uint32_t* out_max_gt, int32_t* out_qphred, int32_t* out_from_ntype_qphred,
                                   uint32_t* out_ntype)
{
    const float neg_inf = -INFINITY;
    const float ln_one_half = (float)log(1. / 2.);
    const float log_error_mod = (float)(-log((double)(PRESTRAND - 1)));
    const float RATIO_INCREMENT = 0.5f / (float)(HET_RES + 1);

    double log_post_prob[SOM_SIZE][2];
    double max_log_prob = neg_inf;
    uint32_t max_gt = 0;

    for (unsigned ngt = 0; ngt < SOM_SIZE; ++ngt) {
        for (unsigned tgt = 0; tgt < 2; ++tgt) {
            double max_log_sum = neg_inf;
            double log_sum[PRESTRAND * PRESTRAND];
            int index = 0;
            for (unsigned tfi = 0; tfi < PRESTRAND; ++tfi) {
                const float tumor_freq = get_fraction_from_index((int)tfi);
                const int consider_norm_contam = (contam_tolerance * tumor_freq >= RATIO_INCREMENT);
                for (unsigned nfi = 0; nfi < PRESTRAND; ++nfi) {
                    double lprior_freq;
                    if (tgt == 0) {
                        if (nfi != tfi) continue;
                        lprior_freq = (nfi == ngt) ? logSharedErrorRateComplement : logSharedErrorRate + log_error_mod;
                    } else {
                        if (nfi == tfi) continue;
                        if (ngt != SOM_REF) {
                            if (nfi != ngt) continue;
                            lprior_freq = log_error_mod;
                        } else {
                            if (!consider_norm_contam) {
                                if (nfi == 0) lprior_freq = log_error_mod;
                                else continue;
                            } else {
                                if ((nfi == ngt) || (nfi == SOM_SIZE)) lprior_freq = log_error_mod + ln_one_half;
                                else continue;
                            }
                        }
                    }
                    const double lsum = lprior_freq + normal_lhood[nfi] + tumor_lhood[tfi];
                    log_sum[index++] = lsum;
                    if (lsum > max_log_sum) max_log_sum = lsum;
                }
            }
            double sum = 0.0;
            for (int i = 0; i < index; ++i) sum += exp(log_sum[i] - max_log_sum);
            const double log_genotype_prior = germlineGenotypeLogPrior[ngt] + ((tgt == 0) ? lnmatch : lnmismatch);
            log_post_prob[ngt][tgt] = log_genotype_prior + max_log_sum + log(sum);
            if (log_post_prob[ngt][tgt] > max_log_prob) {
                max_log_prob = log_post_prob[ngt][tgt];
                max_gt = ngt * 2 + tgt; /* DDIGT::get_state (strelka_digt_states.hh) */
            }
        }
    }

    double sum_prob = 0.0;
    for (unsigned ngt = 0; ngt < SOM_SIZE; ++ngt)
        for (unsigned tgt = 0; tgt < 2; ++tgt) sum_prob += exp(log_post_prob[ngt][tgt] - max_log_prob);
    const double log_sum_prob = log(sum_prob);
    double min_not_somfrom_sum = INFINITY;
    double nonsom_prob = 0.0;
    int32_t from_ntype_qphred = 0;
    uint32_t ntype = 0;
    for (unsigned ngt = 0; ngt < SOM_SIZE; ++ngt) {
        double som_prob_given_ngt = 0;
        for (unsigned tgt = 0; tgt < 2; ++tgt) {
            const double pp = exp(log_post_prob[ngt][tgt] - max_log_prob - log_sum_prob);
            if (tgt == 0) nonsom_prob += pp;
            else som_prob_given_ngt += pp;
        }
        const double err_som_and_ngt = 1.0 - som_prob_given_ngt;
        if (err_som_and_ngt < min_not_somfrom_sum) {
            min_not_somfrom_sum = err_som_and_ngt;
            from_ntype_qphred = sko_error_prob_to_qphred(err_som_and_ngt);
            ntype = ngt;
        }
    }
    *out_max_gt = max_gt;
    *out_qphred = sko_error_prob_to_qphred(nonsom_prob);
    *out_from_ntype_qphred = from_ntype_qphred;
    *out_ntype = ntype;
}

/* snp_pos_info::get_most_frequent_alt_id (L/blt_common/snp_pos_info.hh:164-190) */
static unsigned most_frequent_alt_id(const uint16_t* calls, int32_t n, unsigned ref_gt)
{
    unsigned alt_count[5] = { 0, 0, 0, 0, 0 };
    for (int i = 0; i < n; ++i) {
        const unsigned obs = C_BASE(calls[i]);
        if (obs == ref_gt || obs == 4) continue;
        ++alt_count[obs];
    }
    unsigned alt_id = ref_gt, max_count = 0;
    for (unsigned b = 0; b < 5; ++b) {
        if (alt_count[b] > max_count) {
            if (b == ref_gt) continue;
            max_count = alt_count[b];
            alt_id = b;
        }
    }
    return alt_id;
}

/* position_somatic_snv_call, tier1 only (L/applications/strelka/position_somatic_snv_strand_grid.cpp:230-363) with the
 * constructor's derived parameters (:42-54) and the sb part of the wrapper (:216-225) */
void sko_position_somatic_snv_call(const uint16_t* ncalls, int32_t n_n, const uint16_t* tcalls, int32_t n_t,
                                   uint32_t ref_base_id, const sko_somatic_snv_options* opt, int is_forced_output,
                                   sko_somatic_snv_call* out)
{
    memset(out, 0, sizeof(*out));
    if (ref_base_id >= 4) return;
    if (!is_forced_output) {
        int allref = 1;
        for (int i = 0; i < n_n && allref; ++i) if (C_BASE(ncalls[i]) != ref_base_id) allref = 0;
        for (int i = 0; i < n_t && allref; ++i) if (C_BASE(tcalls[i]) != ref_base_id) allref = 0;
        if (allref) return;
    }
    out->is_called = 1;

    const float contam_tolerance = (float)opt->ssnv_contam_tolerance;
    const float ln_csse_rate = (float)sko_log1p_switch(-opt->shared_site_error_rate);
    const float ln_som_match = (float)sko_log1p_switch(-opt->somatic_snv_rate);
    const float ln_som_mismatch = (float)log(opt->somatic_snv_rate);
    float lnprior[3]; /* calculateGermlineGenotypeLogPrior, qscore_calculator.cpp:35-43 */
    lnprior[SOM_REF] = (float)sko_log1p_switch(-(3. * opt->bsnp_diploid_theta) / 2.);
    lnprior[SOM_HOM] = (float)log(opt->bsnp_diploid_theta / 2.);
    lnprior[SOM_HET] = (float)log(opt->bsnp_diploid_theta);
    const float strand_sse_rate = (float)(opt->shared_site_error_rate * opt->shared_site_error_strand_bias_fraction);
    const float nostrand_sse_rate = (float)(opt->shared_site_error_rate - strand_sse_rate);
    const float ln_sse_rate = logf(nostrand_sse_rate);

    sko_somatic_sample_lhood(ncalls, n_n, ref_base_id, 0, out->normal_lhood);
    sko_somatic_sample_lhood(tcalls, n_t, ref_base_id, 1, out->tumor_lhood);

    sko_calculate_result_set_grid(contam_tolerance, ln_sse_rate, ln_csse_rate, out->normal_lhood, out->tumor_lhood,
                                  lnprior, ln_som_match, ln_som_mismatch, &out->max_gt, &out->qphred,
                                  &out->from_ntype_qphred, &out->ntype);
    out->normal_alt_id = most_frequent_alt_id(ncalls, n_n, ref_base_id);
    out->tumor_alt_id = most_frequent_alt_id(tcalls, n_t, ref_base_id);
    if (!is_forced_output && out->qphred == 0) {
        /* wrapper returns before the strand-bias block (:184) and the caller drops the site (:315-319) */
        out->strand_bias = 0;
        return;
    }
    {
        float symm = out->tumor_lhood[SOM_SIZE];
        for (int i = SOM_SIZE; i < PRESTRAND; ++i) if (symm < out->tumor_lhood[i]) symm = out->tumor_lhood[i];
        float strand = out->tumor_lhood[PRESTRAND];
        for (int i = PRESTRAND; i < GRID; ++i) if (strand < out->tumor_lhood[i]) strand = out->tumor_lhood[i];
        const float d = strand - symm;
        out->strand_bias = (0.f < d) ? d : 0.f;
    }
}

/* ---- the whole of position_somatic_snv_call: both tiers, forced output, non-somatic quality ----
 * (L/applications/strelka/position_somatic_snv_strand_grid.cpp:230-363 with the wrapper calculate_result_set_grid
 * :159-226, gvcf_nonsomatic_gvcf_prior :120-155, isValidNonsomaticIndex :93-113) */

typedef struct tier_result { /* snv_result_set, somatic_result_set.hh:32-54 */
    uint32_t ntype, max_gt;
    int32_t qphred, from_ntype_qphred;
    uint32_t normal_alt_id, tumor_alt_id;
    int32_t nonsomatic_qphred;
    double strandBias;
} tier_result;

static int is_valid_nonsomatic_index(unsigned f)
{
    static const float nonSomaticMinFrac = 0.1f;
    const float nonSomaticMinFracComp = (float)(1. - nonSomaticMinFrac); /* blt_float_t(1.-nonSomaticMinFrac) */
    static const float epsilon = 0.0001f;
    const float nonSomaticMinFracEps = nonSomaticMinFrac - epsilon;
    const float nonSomaticMinFracCompEps = nonSomaticMinFracComp + epsilon;
    if (f == SOM_REF || f == SOM_HOM) return 1;
    const float frac = get_fraction_from_index((int)f);
    if (frac < nonSomaticMinFracEps) return 0;
    if (frac > nonSomaticMinFracCompEps) return 0;
    return 1;
}

static float gvcf_nonsomatic_gvcf_prior(unsigned fn, unsigned ft)
{
    const float lzero = -INFINITY;
    if (!is_valid_nonsomatic_index(ft)) return lzero;
    if (fn == ft) return logf(1.f);
    if (fn == SOM_REF || fn == SOM_HOM) return logf(0.5f);
    return lzero;
}

/* the non-somatic quality block of the wrapper (:186-214), opt_normalize_ln_distro from L/blt_util/prob_util.hh:248-311
 * (its "opt max" is compared against the running max that has just been updated, so it ends up being the first
 * predicate-true entry -- restated as written) */
int sko_nonsomatic_qphred(const float* normal_lhood, const float* tumor_lhood)
{
    enum { N = PRESTRAND * PRESTRAND };
    double pprob[N];
    unsigned char pred[N];
    for (unsigned i = 0; i < N; ++i) pred[i] = 0;
    for (unsigned gt = 0; gt < PRESTRAND; ++gt) pred[gt + PRESTRAND * gt] = 1; /* DDIGT_GRID::is_nonsom, strelka_digt_states.cpp:154-162 */
    for (unsigned fn = 0; fn < PRESTRAND; ++fn)
        for (unsigned ft = 0; ft < PRESTRAND; ++ft) {
            const float v = normal_lhood[fn] + tumor_lhood[ft] + gvcf_nonsomatic_gvcf_prior(fn, ft);
            pprob[fn + PRESTRAND * ft] = v;
        }
    int is_max = 0, is_opt_max = 0;
    double max = 0, opt_max = 0;
    for (unsigned i = 0; i < N; ++i) {
        if ((!is_max) || (pprob[i] > max)) { max = pprob[i]; is_max = 1; }
        if (((!is_opt_max) || (pprob[i] > max)) && pred[i]) { opt_max = pprob[i]; is_opt_max = 1; }
    }
    static const double norm_thresh = 20, opt_thresh = 5;
    double sum = 0.;
    for (unsigned i = 0; i < N; ++i) {
        const double mdiff = max - pprob[i];
        if (mdiff > norm_thresh) {
            if (!pred[i]) { pprob[i] = 0; continue; }
            const double optdiff = opt_max - pprob[i];
            if (optdiff > opt_thresh) { pprob[i] = 0; continue; }
        }
        pprob[i] = exp(-mdiff);
        sum += pprob[i];
    }
    sum = 1. / sum;
    for (unsigned i = 0; i < N; ++i) pprob[i] *= sum;
    double nonsomatic_sum = 0;
    for (unsigned f = 0; f < PRESTRAND; ++f) nonsomatic_sum += pprob[f + PRESTRAND * f];
    return sko_error_prob_to_qphred(1. - nonsomatic_sum);
}

void sko_position_somatic_snv_call_tiers(const uint16_t* n1, int32_t n_n1, const uint16_t* t1, int32_t n_t1,
                                         const uint16_t* n2, int32_t n_n2, const uint16_t* t2, int32_t n_t2, int is_tier2,
                                         uint32_t ref_base_id, const sko_somatic_snv_options* opt, int is_forced_output,
                                         int is_compute_nonsomatic, sko_somatic_snv_genotype* sgt)
{
    memset(sgt, 0, sizeof(*sgt));
    sgt->is_forced_output = (uint8_t)(is_forced_output ? 1 : 0);
    if (ref_base_id >= 4) { /* :244-248 */
        sgt->is_forced_output = 0;
        return;
    }
    sgt->ref_gt = ref_base_id;
    if (!(is_forced_output || is_compute_nonsomatic)) { /* :251-254, tier1 pileups */
        int allref = 1;
        for (int i = 0; i < n_n1 && allref; ++i) if (C_BASE(n1[i]) != ref_base_id) allref = 0;
        for (int i = 0; i < n_t1 && allref; ++i) if (C_BASE(t1[i]) != ref_base_id) allref = 0;
        if (allref) return;
    }
    sgt->is_computed = 1;

    const float contam_tolerance = (float)opt->ssnv_contam_tolerance;
    const float ln_csse_rate = (float)sko_log1p_switch(-opt->shared_site_error_rate);
    const float ln_som_match = (float)sko_log1p_switch(-opt->somatic_snv_rate);
    const float ln_som_mismatch = (float)log(opt->somatic_snv_rate);
    float lnprior[3];
    lnprior[SOM_REF] = (float)sko_log1p_switch(-(3. * opt->bsnp_diploid_theta) / 2.);
    lnprior[SOM_HOM] = (float)log(opt->bsnp_diploid_theta / 2.);
    lnprior[SOM_HET] = (float)log(opt->bsnp_diploid_theta);
    const float strand_sse_rate = (float)(opt->shared_site_error_rate * opt->shared_site_error_strand_bias_fraction);
    const float nostrand_sse_rate = (float)(opt->shared_site_error_rate - strand_sse_rate);
    const float ln_sse_rate = logf(nostrand_sse_rate);

    tier_result tier_rs[2];
    memset(tier_rs, 0, sizeof(tier_rs));
    for (unsigned i = 0; i < 2; ++i) {
        const int is_include_tier2 = (i == 1);
        if (is_include_tier2) {
            if (!is_tier2) continue;
            if (tier_rs[0].qphred == 0) { tier_rs[1] = tier_rs[0]; continue; }
        }
        const uint16_t* nc = is_include_tier2 ? n2 : n1;
        const uint16_t* tc = is_include_tier2 ? t2 : t1;
        const int32_t nn = is_include_tier2 ? n_n2 : n_n1, nt = is_include_tier2 ? n_t2 : n_t1;
        float normal_lhood[GRID], tumor_lhood[GRID];
        sko_somatic_sample_lhood(nc, nn, ref_base_id, 0, normal_lhood);
        sko_somatic_sample_lhood(tc, nt, ref_base_id, 1, tumor_lhood);
        tier_result* rs = &tier_rs[i];
        sko_calculate_result_set_grid(contam_tolerance, ln_sse_rate, ln_csse_rate, normal_lhood, tumor_lhood, lnprior,
                                      ln_som_match, ln_som_mismatch, &rs->max_gt, &rs->qphred, &rs->from_ntype_qphred,
                                      &rs->ntype);
        if ((is_forced_output || is_compute_nonsomatic) || rs->qphred != 0) { /* wrapper :184 */
            if (is_compute_nonsomatic) rs->nonsomatic_qphred = sko_nonsomatic_qphred(normal_lhood, tumor_lhood);
            float symm = tumor_lhood[SOM_SIZE];
            for (int k = SOM_SIZE; k < PRESTRAND; ++k) if (symm < tumor_lhood[k]) symm = tumor_lhood[k];
            float strand = tumor_lhood[PRESTRAND];
            for (int k = PRESTRAND; k < GRID; ++k) if (strand < tumor_lhood[k]) strand = tumor_lhood[k];
            const float d = strand - symm;
            rs->strandBias = (0.f < d) ? d : 0.f;
        }
        rs->normal_alt_id = most_frequent_alt_id(nc, nn, ref_base_id);
        rs->tumor_alt_id = most_frequent_alt_id(tc, nt, ref_base_id);
    }
    if (!(is_forced_output || is_compute_nonsomatic)) { /* :315-319 */
        if ((tier_rs[0].qphred == 0) || (is_tier2 && (tier_rs[1].qphred == 0))) return;
    }
    sgt->snv_tier = 0;
    sgt->snv_from_ntype_tier = 0;
    if (is_tier2) {
        if (tier_rs[0].qphred > tier_rs[1].qphred) sgt->snv_tier = 1;
        if (tier_rs[0].from_ntype_qphred > tier_rs[1].from_ntype_qphred) sgt->snv_from_ntype_tier = 1;
    }
    const tier_result* rs = &tier_rs[sgt->snv_from_ntype_tier];
    sgt->ntype = rs->ntype;
    sgt->max_gt = rs->max_gt;
    sgt->from_ntype_qphred = rs->from_ntype_qphred;
    sgt->normal_alt_id = rs->normal_alt_id;
    sgt->tumor_alt_id = rs->tumor_alt_id;
    sgt->strand_bias = rs->strandBias;
    if (is_tier2 && (tier_rs[0].ntype != tier_rs[1].ntype)) { /* NTYPE::CONFLICT, somatic_call_shared.hh:32-40 */
        sgt->ntype = 3;
        sgt->from_ntype_qphred = 0;
    } else {
        if (sgt->ntype == SOM_REF) sgt->ntype = 0;
        else if (sgt->ntype == SOM_HOM) sgt->ntype = 1;
        else sgt->ntype = 2;
    }
    sgt->qphred = tier_rs[sgt->snv_tier].qphred;
    sgt->nonsomatic_qphred = tier_rs[0].nonsomatic_qphred;
}

/* ------------------------------------------------------------------------------------ hot path B: indels */

/* get_het_observed_allele_ratio, L/starling_common/starling_indel_call_pprob_digt.cpp:40-71 */
void sko_het_observed_allele_ratio(unsigned read_length, unsigned min_overlap, unsigned del_len, unsigned ins_len,
                                   double het_allele_ratio, double* log_ref_prob, double* log_indel_prob)
{
    const unsigned base_expect = ((read_length + 1) < (2 * min_overlap)) ? 0 : (read_length + 1) - (2 * min_overlap);
    const double ref_path_expect = base_expect + ((del_len < base_expect) ? del_len : base_expect);
    const double indel_path_expect = base_expect + ((ins_len < base_expect) ? ins_len : base_expect);
    const double ref_path_term = (1 - het_allele_ratio) * ref_path_expect;
    const double indel_path_term = het_allele_ratio * indel_path_expect;
    const double total_path_term = ref_path_term + indel_path_term;
    if (total_path_term > 0) {
        const double indel_prob = indel_path_term / total_path_term;
        *log_ref_prob = log(1. - indel_prob);
        *log_indel_prob = log(indel_prob);
    }
}

/* integrateOutMappingStatus, L/starling_common/readMappingAdjustmentUtil.hh:29-56 */
double sko_integrate_out_mapping_status(double randomBaseMatchLogProb, unsigned nonAmbiguousBasesInRead, double lnp)
{
    const double correctMappingLogPrior = log(1.7e-10); /* starling_base_shared.cpp:64 */
    return sko_log_sum2(lnp + correctMappingLogPrior, randomBaseMatchLogProb * nonAmbiguousBasesInRead);
}

void sko_indel_grid_lhood(int32_t n_reads, const float* ref_lnp, const float* indel_lnp, const float* alt_lnp,
                          const uint16_t* non_ambig, const uint16_t* read_length, const uint8_t* is_tier1,
                          unsigned del_len, unsigned ins_len, int is_breakpoint, int min_read_bp_flank,
                          double randomBaseMatchProb, int is_include_tier2, int is_use_alt_indel, double* lhood)
{
    const double rbm = log(randomBaseMatchProb); /* starling_base_shared.cpp:42 */
    const float RATIO_INCREMENT = 0.5f / (float)(HET_RES + 1);
    for (int i = 0; i < PRESTRAND; ++i) lhood[i] = 0.;

    /* get_indel_digt_lhood :240-310 : STAR_DIINDEL NOINDEL=0, HOM=1, HET=2 (== SOMATIC_DIGT REF, HOM, HET) */
    const double loghalf = -log(2.);
    for (int r = 0; r < n_reads; ++r) {
        if ((!is_include_tier2) && (!is_tier1[r])) continue;
        double alt_path_lnp = ref_lnp[r];
        if (is_use_alt_indel && alt_lnp[r] == alt_lnp[r] && alt_lnp[r] > alt_path_lnp) alt_path_lnp = alt_lnp[r];
        const double noindel_lnp = alt_path_lnp;
        const double hom_lnp = indel_lnp[r];
        double log_ref_prob = loghalf, log_indel_prob = loghalf;
        if (!is_breakpoint)
            sko_het_observed_allele_ratio(read_length[r], (unsigned)min_read_bp_flank, del_len, ins_len, 0.5,
                                          &log_ref_prob, &log_indel_prob);
        const double het_lnp = sko_log_sum2(noindel_lnp + log_ref_prob, hom_lnp + log_indel_prob);
        lhood[SOM_REF] += sko_integrate_out_mapping_status(rbm, non_ambig[r], noindel_lnp);
        lhood[SOM_HOM] += sko_integrate_out_mapping_status(rbm, non_ambig[r], hom_lnp);
        lhood[SOM_HET] += sko_integrate_out_mapping_status(rbm, non_ambig[r], het_lnp);
    }

    /* get_indel_het_grid_lhood (somatic_indel_grid.cpp:66-89) over get_high_low_het_ratio_lhood (:75-155) */
    double* grid = lhood + SOM_SIZE;
    const unsigned lsize = HET_RES * 2;
    for (unsigned i = 0; i < HET_RES; ++i) {
        const double het_ratio = (i + 1) * RATIO_INCREMENT; /* unsigned * float -> float, widened */
        const double chet_ratio = 1. - het_ratio;
        const double log_het_ratio = log(het_ratio);
        const double log_chet_ratio = log(chet_ratio);
        double het_lhood_high = 0, het_lhood_low = 0;
        for (int r = 0; r < n_reads; ++r) {
            if ((!is_include_tier2) && (!is_tier1[r])) continue;
            double alt_path_lnp = ref_lnp[r];
            if (is_use_alt_indel && alt_lnp[r] == alt_lnp[r] && alt_lnp[r] > alt_path_lnp) alt_path_lnp = alt_lnp[r];
            const double noindel_lnp = alt_path_lnp;
            const double hom_lnp = indel_lnp[r];
            {
                double log_ref_prob = log_chet_ratio, log_indel_prob = log_het_ratio;
                if (!is_breakpoint)
                    sko_het_observed_allele_ratio(read_length[r], (unsigned)min_read_bp_flank, del_len, ins_len,
                                                  het_ratio, &log_ref_prob, &log_indel_prob);
                const double het_lnp = sko_log_sum2(noindel_lnp + log_ref_prob, hom_lnp + log_indel_prob);
                het_lhood_low += sko_integrate_out_mapping_status(rbm, non_ambig[r], het_lnp);
            }
            {
                double log_ref_prob = log_het_ratio, log_indel_prob = log_chet_ratio;
                if (!is_breakpoint)
                    sko_het_observed_allele_ratio(read_length[r], (unsigned)min_read_bp_flank, del_len, ins_len,
                                                  chet_ratio, &log_ref_prob, &log_indel_prob);
                const double het_lnp = sko_log_sum2(noindel_lnp + log_ref_prob, hom_lnp + log_indel_prob);
                het_lhood_high += sko_integrate_out_mapping_status(rbm, non_ambig[r], het_lnp);
            }
        }
        grid[lsize - (i + 1)] = het_lhood_high;
        grid[i] = het_lhood_low;
    }
}

void sko_allele_group_genotype_lhoods(int32_t n_reads, int32_t n_alt, const float* ref_lnp, const float* allele_lnp,
                                      const uint16_t* non_ambig, const uint16_t* read_length, const uint8_t* is_tier1,
                                      const uint8_t* is_fwd, const uint32_t* del_len, const uint32_t* ins_len,
                                      int ploidy, int min_read_bp_flank, double randomBaseMatchProb,
                                      double readSupportThreshold, double* out_lhood, uint32_t* out_counts)
{
    const double rbm = log(randomBaseMatchProb);
    const int full = n_alt + 1;
    const int gcount = (ploidy == 1) ? full : full * (full + 1) / 2;
    for (int g = 0; g < gcount; ++g) out_lhood[g] = 0.;
    memset(out_counts, 0, sizeof(uint32_t) * 2 * (size_t)(n_alt + 2));
    if (n_alt <= 0) return;
    double L[18], Lm[18]; /* (up to SK_MAX_ALT_XWIDE = 16 alternate alleles + the reference) */
    assert(full <= 18);
    for (int r = 0; r < n_reads; ++r) {
        /* getAlleleGroupIntersectionReadIds (OrthogonalVariantAlleleCandidateGroupUtil.cpp:64-113), tier1 only:
         * the read must be scored for every allele of the group */
        int present = 0;
        for (int a = 0; a < n_alt; ++a) {
            const float s = allele_lnp[r * n_alt + a];
            if (s == s && is_tier1[r]) ++present;
        }
        if (present < n_alt) continue;
        /* getAlleleLogLhoodFromRead (:132-197) */
        for (int a = 0; a < n_alt; ++a) {
            const double rl = (double)ref_lnp[r * n_alt + a];
            if (a == 0) L[0] = rl;
            else L[0] = (L[0] < rl) ? rl : L[0];
            L[a + 1] = allele_lnp[r * n_alt + a];
        }
        /* updateGenotypeLogLhoodFromAlleleLogLhood (AlleleGroupGenotype.cpp:36-114) */
        if (ploidy == 1) {
            for (int a0 = 0; a0 < full; ++a0) out_lhood[a0] += sko_integrate_out_mapping_status(rbm, non_ambig[r], L[a0]);
        } else {
            for (int a1 = 0; a1 < full; ++a1) {
                for (int a0 = 0; a0 <= a1; ++a0) {
                    const int gi = a0 + (a1 * (a1 + 1) / 2);
                    double raw = 0;
                    if (a0 != a1) {
                        const double loghalf = log(0.5);
                        double lp0 = loghalf, lp1 = loghalf;
                        sko_het_observed_allele_ratio(read_length[r], (unsigned)min_read_bp_flank, del_len[a1 - 1],
                                                      ins_len[a1 - 1], 0.5, &lp0, &lp1);
                        if (a0 > 0) {
                            double logRefPrior = loghalf;
                            lp0 = loghalf;
                            sko_het_observed_allele_ratio(read_length[r], (unsigned)min_read_bp_flank, del_len[a0 - 1],
                                                          ins_len[a0 - 1], 0.5, &logRefPrior, &lp0);
                            const double norm = sko_log_sum2(lp0, lp1);
                            lp0 -= norm;
                            lp1 -= norm;
                        }
                        raw = sko_log_sum2(L[a0] + lp0, L[a1] + lp1);
                    } else {
                        raw = L[a0];
                    }
                    out_lhood[gi] += sko_integrate_out_mapping_status(rbm, non_ambig[r], raw);
                }
            }
        }
        /* updateSupportingReadStats (:125-155) */
        for (int a = 0; a < full; ++a) Lm[a] = sko_integrate_out_mapping_status(rbm, non_ambig[r], L[a]);
        {
            double mx = Lm[0];
            for (int a = 1; a < full; ++a) if (Lm[a] > mx) mx = Lm[a];
            double sum = 0.;
            for (int a = 0; a < full; ++a) { Lm[a] = exp(Lm[a] - mx); sum += Lm[a]; }
            sum = 1. / sum;
            for (int a = 0; a < full; ++a) Lm[a] *= sum;
        }
        uint32_t* cnt = out_counts + (is_fwd[r] ? 0 : 1) * (n_alt + 2);
        int found = 0;
        for (int a = 0; a < full; ++a) {
            if (Lm[a] < readSupportThreshold) continue;
            cnt[a]++;
            found = 1;
            break;
        }
        if (!found) cnt[n_alt + 1]++;
    }
}

void sko_somatic_indel_result(const double* normal_lhood, const double* tumor_lhood, double indelToRefErrorProb,
                              double shared_indel_error_factor, double indel_contam_tolerance, double somatic_indel_rate,
                              double bindel_diploid_theta, uint32_t* max_gt, int32_t* qphred, int32_t* from_ntype_qphred,
                              uint32_t* ntype)
{
    float nf[PRESTRAND], tf[PRESTRAND];
    for (int j = 0; j < PRESTRAND; ++j) {
        nf[j] = (float)normal_lhood[j];
        tf[j] = (float)tumor_lhood[j];
    }
    const double sharedIndelErrorRate = pow(indelToRefErrorProb, shared_indel_error_factor);
    const double logSharedIndelErrorRate = log(sharedIndelErrorRate);
    const double logSharedIndelErrorRateComplement = sko_log1p_switch(-sharedIndelErrorRate);
    float lnprior[3]; /* somatic_indel_caller_grid ctor :58-64 */
    lnprior[SOM_REF] = (float)sko_log1p_switch(-(3. * bindel_diploid_theta) / 2.);
    lnprior[SOM_HOM] = (float)log(bindel_diploid_theta / 2.);
    lnprior[SOM_HET] = (float)log(bindel_diploid_theta);
    const float ln_som_match = (float)sko_log1p_switch(-somatic_indel_rate);
    const float ln_som_mismatch = (float)log(somatic_indel_rate);
    sko_calculate_result_set_grid((float)indel_contam_tolerance, (float)logSharedIndelErrorRate,
                                  (float)logSharedIndelErrorRateComplement, nf, tf, lnprior, ln_som_match,
                                  ln_som_mismatch, max_gt, qphred, from_ntype_qphred, ntype);
}

/* ------------------------------------------------------------------------------------------------ batch drivers */

void sko_score_cases(const sko_read_case* cases, int32_t n_cases, double* out)
{
    int64_t k = 0;
    for (int32_t i = 0; i < n_cases; ++i) {
        const sko_read_case* c = &cases[i];
        for (int32_t j = 0; j < c->n_cals; ++j)
            out[k++] = sko_score_candidate_alignment(c->read_code, c->read_qual, c->read_len, &c->cals[j], c->ref_seq,
                                                     c->ref_offset, c->ref_len);
    }
}

void sko_adjust_joint_eprob_batch(const int64_t* call_off, const uint16_t* calls, int32_t n_loci,
                                  const sko_germline_options* opt, float* de)
{
    for (int32_t l = 0; l < n_loci; ++l)
        sko_adjust_joint_eprob(calls + call_off[l], (int32_t)(call_off[l + 1] - call_off[l]), opt, de + call_off[l]);
}

void sko_site_digt_call_batch(const int64_t* call_off, const uint16_t* calls, const float* de, const uint8_t* ref_base,
                              const uint8_t* ploidy, int32_t n_loci, const sko_germline_options* opt, sko_digt_call* out)
{
    for (int32_t l = 0; l < n_loci; ++l)
        sko_position_snp_call_pprob_digt(calls + call_off[l], de + call_off[l], (int32_t)(call_off[l + 1] - call_off[l]),
                                         ref_base[l], ploidy ? ploidy[l] : 2, opt, &out[l]);
}

void sko_somatic_snv_call_batch(const int64_t* n_off, const uint16_t* n_calls, const int64_t* t_off,
                                const uint16_t* t_calls, const uint8_t* ref_base, int32_t n_loci,
                                const sko_somatic_snv_options* opt, int is_forced_output, sko_somatic_snv_call* out)
{
    for (int32_t l = 0; l < n_loci; ++l)
        sko_position_somatic_snv_call(n_calls + n_off[l], (int32_t)(n_off[l + 1] - n_off[l]), t_calls + t_off[l],
                                      (int32_t)(t_off[l + 1] - t_off[l]), ref_base[l], opt, is_forced_output, &out[l]);
}

/* ------------------------------------------------------------------------ the whole of get_somatic_indel (a14) */

/* indel_lnp_to_pprob, L/starling_common/AlleleReportInfoUtil.cpp:220-301.  ReadPathScores::score_t is float: every store
 * to a pprob field rounds to float, the arithmetic in between is double wherever a double operand takes part. */
typedef struct read_pprob {
    float ref, indel;
    int n_alt;
    int32_t alt_key[2];
    float alt[2];
} read_pprob;

static const double CORRECT_MAPPING_LOG_PRIOR_INIT = 0; /* placeholder, see correct_mapping_log_prior() */
static double correct_mapping_log_prior(void)
{
    (void)CORRECT_MAPPING_LOG_PRIOR_INIT;
    return log(1.7e-10); /* starling_base_deriv_options: correctMappingLogPrior, starling_base_shared.cpp:64 */
}

static read_pprob indel_lnp_to_pprob(const sko_indel_sample_reads* s, int r, double random_base_match_log_prob,
                                     int is_use_alt_indel)
{
    read_pprob pp;
    int n_in = 0;
    for (int a = 0; a < 2; ++a) if (s->alt_key[2 * r + a] >= 0) ++n_in;
    unsigned n_alleles = 2;
    if (is_use_alt_indel) n_alleles += (unsigned)n_in;
    const double allele_prior = 1. / (double)n_alleles;
    const double allele_lnprior = log(allele_prior);
    const double cmlp = correct_mapping_log_prior();
    float incorrect = (float)(random_base_match_log_prob * s->non_ambig[r]); /* getIncorrectMappingLogLikelihood -> score_t */
    pp.ref = (float)(s->ref_lnp[r] + cmlp + allele_lnprior);
    pp.indel = (float)(s->indel_lnp[r] + cmlp + allele_lnprior);
    pp.n_alt = 0;
    if (is_use_alt_indel) {
        for (int a = 0; a < n_in; ++a) {
            pp.alt_key[pp.n_alt] = s->alt_key[2 * r + a];
            pp.alt[pp.n_alt] = (float)(s->alt_lnp[2 * r + a] + cmlp + allele_lnprior);
            ++pp.n_alt;
        }
    }
    const float m1 = (pp.ref < pp.indel) ? pp.indel : pp.ref;           /* std::max(pprob.ref,pprob.indel) */
    double scale = (incorrect < m1) ? m1 : incorrect;                   /* std::max(incorrect, ...) -> double */
    for (int a = 0; a < pp.n_alt; ++a) if (scale < pp.alt[a]) scale = pp.alt[a];
    incorrect = (float)exp(incorrect - scale);
    pp.ref = (float)exp(pp.ref - scale);
    pp.indel = (float)exp(pp.indel - scale);
    for (int a = 0; a < pp.n_alt; ++a) pp.alt[a] = (float)exp(pp.alt[a] - scale);
    double sum = incorrect + pp.ref + pp.indel; /* three floats added in float, then widened */
    for (int a = 0; a < pp.n_alt; ++a) sum += pp.alt[a];
    pp.ref = (float)(pp.ref / sum);
    pp.indel = (float)(pp.indel / sum);
    for (int a = 0; a < pp.n_alt; ++a) pp.alt[a] = (float)(pp.alt[a] / sum);
    return pp;
}

typedef struct total_pprob {
    float ref, indel;
    int n_alt, cap;
    int32_t* alt_key;
    float* alt;
} total_pprob;

/* get_sum_path_pprob, L/starling_common/starling_indel_call_pprob_digt.cpp:187-236: the key -> slot map is local to one
 * call, so the tumor sample's alternates are appended after the normal sample's even where the key repeats */
static void sum_path_pprob(const sko_indel_sample_reads* s, double random_base_match_log_prob, int is_tier2_pass,
                           int is_use_alt_indel, total_pprob* t, int is_init_total)
{
    if (is_init_total) { t->ref = 0; t->indel = 0; }
    const int first_slot = t->n_alt;
    for (int r = 0; r < s->n_reads; ++r) {
        if ((!is_tier2_pass) && (!s->is_tier1[r])) continue;
        const read_pprob pp = indel_lnp_to_pprob(s, r, random_base_match_log_prob, is_use_alt_indel);
        t->indel += pp.indel;
        t->ref += pp.ref;
        if (!is_use_alt_indel) continue;
        for (int a = 0; a < pp.n_alt; ++a) {
            int slot = -1;
            for (int k = first_slot; k < t->n_alt; ++k) if (t->alt_key[k] == pp.alt_key[a]) { slot = k; break; }
            if (slot < 0) {
                assert(t->n_alt < t->cap);
                t->alt_key[t->n_alt] = pp.alt_key[a];
                t->alt[t->n_alt] = pp.alt[a];
                ++t->n_alt;
            } else {
                t->alt[slot] += pp.alt[a];
            }
        }
    }
}

static int alt_keys_conflict(const sko_alt_key* a, const sko_alt_key* b) /* is_indel_conflict, indel_util.cpp:27-45 */
{
    const int either_mismatch = a->is_mismatch || b->is_mismatch;
    const int32_t e1 = a->end_pos + (either_mismatch ? 0 : 1), e2 = b->end_pos + (either_mismatch ? 0 : 1);
    return (e2 > a->begin_pos) && (b->begin_pos < e1); /* pr1.is_range_intersect(pr2), pos_range.hh:102-106 */
}

typedef struct score_entry { double score; int id; } score_entry;
static int score_entry_less(const void* x, const void* y)
{
    const score_entry* a = (const score_entry*)x; const score_entry* b = (const score_entry*)y;
    if (a->score < b->score) return -1;
    if (b->score < a->score) return 1;
    return (a->id < b->id) ? -1 : ((b->id < a->id) ? 1 : 0); /* std::pair<double,int> operator< */
}

int sko_is_multi_indel_allele(const sko_indel_sample_reads* normal, const sko_indel_sample_reads* tumor,
                              const sko_alt_key* alt_keys, const sko_somatic_indel_params* p, int is_include_tier2,
                              int* is_overlap)
{
    enum { INDEL_ID = -2, REF_ID = -1 };
    const double rbm = is_include_tier2 ? log(p->tier2_random_base_match_prob) : log(p->random_base_match_prob);
    total_pprob t;
    const int cap = 2 * (normal->n_reads + tumor->n_reads) + 1;
    t.alt_key = (int32_t*)malloc(sizeof(int32_t) * (size_t)cap);
    t.alt = (float*)malloc(sizeof(float) * (size_t)cap);
    t.n_alt = 0; t.cap = cap; t.ref = 0; t.indel = 0;
    sum_path_pprob(normal, rbm, is_include_tier2, 1, &t, 1);
    sum_path_pprob(tumor, rbm, is_include_tier2, 1, &t, 0);
    int n = 2 + t.n_alt;
    score_entry* scores = (score_entry*)malloc(sizeof(score_entry) * (size_t)n);
    scores[0].score = -t.indel; scores[0].id = INDEL_ID;
    scores[1].score = -t.ref; scores[1].id = REF_ID;
    for (int i = 0; i < t.n_alt; ++i) { scores[2 + i].score = -t.alt[i]; scores[2 + i].id = i; }
    qsort(scores, (size_t)n, sizeof(score_entry), score_entry_less); /* total order: equal to std::sort's result */
    while (scores[0].id >= 0 && scores[1].id >= 0) {
        if (alt_keys_conflict(&alt_keys[t.alt_key[scores[0].id]], &alt_keys[t.alt_key[scores[1].id]])) break;
        memmove(scores + 1, scores + 2, sizeof(score_entry) * (size_t)(n - 2));
        --n;
    }
    int result = 0;
    if ((scores[0].id != INDEL_ID) && (scores[1].id != INDEL_ID)) result = 1;
    if (!result && n >= 3) {
        const double top_prob = scores[0].score + scores[1].score;
        const double top_frac = top_prob / (top_prob + scores[2].score);
        if (top_frac < .9) result = 1;
    }
    if (!result) *is_overlap = ((scores[0].id != REF_ID) && (scores[1].id != REF_ID));
    free(scores); free(t.alt_key); free(t.alt);
    return result;
}

void sko_get_somatic_indel(const sko_indel_sample_reads* normal, const sko_indel_sample_reads* tumor,
                           const sko_alt_key* alt_keys, int32_t n_alt_keys, unsigned del_len, unsigned ins_len,
                           int is_breakpoint, const sko_somatic_indel_params* p, double indel_to_ref_error_prob,
                           int is_forced_output, sko_somatic_indel_genotype* out)
{
    (void)n_alt_keys;
    memset(out, 0, sizeof(*out));
    out->is_forced_output = (uint8_t)(is_forced_output ? 1 : 0);
    struct { uint32_t ntype, max_gt; int32_t qphred, from_ntype_qphred; int is_overlap; } tier_rs[2];
    memset(tier_rs, 0, sizeof(tier_rs)); /* the reference leaves ntype / max_gt of a skipped tier indeterminate: 0 here */

    /* per-read best alternate score for the likelihood functions (get_indel_digt_lhood reads path_lnp.alt_indel's max) */
    const sko_indel_sample_reads* smp[2] = { normal, tumor };
    float* alt_max[2];
    for (int s = 0; s < 2; ++s) {
        alt_max[s] = (float*)malloc(sizeof(float) * (size_t)(smp[s]->n_reads + 1));
        for (int r = 0; r < smp[s]->n_reads; ++r) {
            float m = NAN;
            for (int a = 0; a < 2; ++a) {
                if (smp[s]->alt_key[2 * r + a] < 0) continue;
                const float v = smp[s]->alt_lnp[2 * r + a];
                if (!(m == m) || m < v) m = v;
            }
            alt_max[s][r] = m;
        }
    }

    for (unsigned i = 0; i < 2; ++i) {
        const int is_include_tier2 = (i == 1);
        if (is_include_tier2) {
            if (!p->use_tier2_evidence) continue;
            if (tier_rs[0].qphred == 0) {
                if (!is_forced_output) { tier_rs[1].qphred = 0; continue; }
            }
        }
        int is_overlap = tier_rs[i].is_overlap;
        const int is_filter = sko_is_multi_indel_allele(normal, tumor, alt_keys, p, is_include_tier2, &is_overlap);
        tier_rs[i].is_overlap = is_overlap;
        if (is_filter && !is_forced_output) { tier_rs[i].qphred = 0; continue; }

        double normal_lhood[PRESTRAND], tumor_lhood[PRESTRAND];
        const double rbm = is_include_tier2 ? p->tier2_random_base_match_prob : p->random_base_match_prob;
        sko_indel_grid_lhood(normal->n_reads, normal->ref_lnp, normal->indel_lnp, alt_max[0], normal->non_ambig,
                             normal->read_length, normal->is_tier1, del_len, ins_len, is_breakpoint,
                             p->normal_min_read_bp_flank, rbm, is_include_tier2, p->is_use_alt_indel, normal_lhood);
        sko_indel_grid_lhood(tumor->n_reads, tumor->ref_lnp, tumor->indel_lnp, alt_max[1], tumor->non_ambig,
                             tumor->read_length, tumor->is_tier1, del_len, ins_len, is_breakpoint,
                             p->tumor_min_read_bp_flank, rbm, is_include_tier2, p->is_use_alt_indel, tumor_lhood);
        sko_somatic_indel_result(normal_lhood, tumor_lhood, indel_to_ref_error_prob, p->shared_indel_error_factor,
                                 p->indel_contam_tolerance, p->somatic_indel_rate, p->bindel_diploid_theta,
                                 &tier_rs[i].max_gt, &tier_rs[i].qphred, &tier_rs[i].from_ntype_qphred, &tier_rs[i].ntype);
        if (is_filter) tier_rs[i].qphred = 0;
    }
    free(alt_max[0]); free(alt_max[1]);

    if (!is_forced_output) {
        if (tier_rs[0].qphred == 0 || tier_rs[1].qphred == 0) return;
    }
    out->sindel_tier = 0;
    if (p->use_tier2_evidence && (tier_rs[0].qphred > tier_rs[1].qphred)) out->sindel_tier = 1;
    out->sindel_from_ntype_tier = 0;
    if (p->use_tier2_evidence && (tier_rs[0].from_ntype_qphred > tier_rs[1].from_ntype_qphred)) out->sindel_from_ntype_tier = 1;
    const unsigned ft = out->sindel_from_ntype_tier;
    out->ntype = tier_rs[ft].ntype;
    out->max_gt = tier_rs[ft].max_gt;
    out->from_ntype_qphred = tier_rs[ft].from_ntype_qphred;
    out->is_overlap = (uint8_t)(tier_rs[ft].is_overlap ? 1 : 0);
    if (tier_rs[0].ntype != tier_rs[1].ntype) {
        out->ntype = 3; /* NTYPE::CONFLICT */
        out->from_ntype_qphred = 0;
    } else {
        if (out->ntype == SOM_REF) out->ntype = 0;
        else if (out->ntype == SOM_HOM) out->ntype = 1;
        else out->ntype = 2;
    }
    out->qphred = tier_rs[out->sindel_tier].qphred;
}

/* ---------------------------------------------------------------------------------------------------- row a8: pileup */

/* qphred_cache::mappedq, L/blt_util/qscore_cache.cpp:46-49 with phred_to_mapped_error_prob (qscore.hh:104-113) */
int sko_mapped_qscore(int basecall_q, int mapq)
{
    if (mapq > 90) mapq = 90; /* MAX_MAP, qscore_cache.hh:129-132 */
    const double be = pow(10., -((double)basecall_q) / 10.);
    const double me = pow(10., -((double)mapq) / 10.);
    return sko_error_prob_to_qphred(((1. - me) * be) + (me * 0.75));
}

static int pl_seg_match(uint32_t t) { return t == 1 || t == 8 || t == 9; }              /* is_segment_align_match */
static int pl_seg_read_len(uint32_t t) { return pl_seg_match(t) || t == 2 || t == 5; }   /* MATCH-likes, INSERT, SOFT_CLIP */
static int pl_seg_ref_len(uint32_t t) { return pl_seg_match(t) || t == 3 || t == 4; }    /* MATCH-likes, DELETE, SKIP */

static char pl_ref_char(const sko_read_batch* b, int p)
{
    if (p < b->ref_offset || p >= b->ref_offset + b->ref_len) return 'N'; /* reference_contig_segment::get_base */
    return b->ref_seq[p - b->ref_offset];
}
static char pl_code_char(uint8_t c)
{
    switch (c) {
    case 0: return '=';
    case 1: return 'A';
    case 2: return 'C';
    case 4: return 'G';
    case 8: return 'T';
    default: return 'N';
    }
}

typedef struct pl_col {
    uint16_t* v;
    int32_t n, cap;
} pl_col;
static int pl_push(pl_col* c, uint16_t x)
{
    if (c->n == c->cap) {
        const int32_t nc = c->cap ? 2 * c->cap : 16;
        uint16_t* nv = (uint16_t*)realloc(c->v, sizeof(uint16_t) * (size_t)nc);
        if (!nv) return 1;
        c->v = nv;
        c->cap = nc;
    }
    c->v[c->n++] = x;
    return 0;
}

int64_t sko_pileup_reads(const sko_read_batch* b, const sko_pileup_options* o, int mode, int64_t* call_off,
                         uint16_t* calls, int64_t capacity, uint32_t* spandel_count, uint32_t* submapped_count)
{
    return sko_pileup_reads_mapq(b, o, mode, call_off, calls, capacity, spandel_count, submapped_count, NULL, NULL, NULL);
}

/* the same with the MapqTracker of every position (insert_mapq_count, starling_pos_processor_base.cpp:1346:
 * every match position inside the trimmed read and the report range, submapped reads included;
 * L/blt_common/MapqTracker.hh:36-42) */
static int64_t pileup_reads_impl(const sko_read_batch* b, const sko_pileup_options* o, int mode, int64_t* call_off,
                                 uint16_t* calls, int64_t capacity, uint32_t* spandel_count, uint32_t* submapped_count,
                                 uint32_t* mapq_count, uint32_t* mapq_zero_count, uint64_t* mapq_sum_square, uint32_t* read_pos);
static int64_t g_evs_capacity = 0; /* sko_pileup_reads_evs's side outputs (test infrastructure: single-threaded) */
static int64_t* g_evs_off = NULL;
static uint64_t* g_evs_words = NULL;

/* What updateGermlineScoringMetrics gets (L/starling_common/starling_pos_processor_base.cpp:1346-1357 ->
 * pos_basecall_buffer.cpp:43-70) for every live match position of every read, submapped reads included, in pileup order, one
 * word each: base id (bits 0-2) | mapq << 3 | qscore << 11 (after the MAPQ adjustment, not capped) | cycle << 18
 * (align_strand_read_pos) | min(20, distance from the read edge) << 29 | is_submapped << 34.  evs_off[n_loci + 1]. */
int64_t sko_pileup_reads_evs(const sko_read_batch* b, const sko_pileup_options* o, int64_t* evs_off, uint64_t* evs_words, int64_t capacity)
{
    const int32_t n_loci = o->report_end - o->report_begin;
    int64_t* off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_loci + 1));
    uint16_t* calls = (uint16_t*)malloc(sizeof(uint16_t) * (size_t)(capacity + 1));
    g_evs_capacity = capacity;
    g_evs_off = evs_off;
    g_evs_words = evs_words;
    const int64_t rc = pileup_reads_impl(b, o, 0, off, calls, capacity, NULL, NULL, NULL, NULL, NULL, NULL);
    g_evs_off = NULL;
    g_evs_words = NULL;
    free(off);
    free(calls);
    return rc < 0 ? rc : evs_off[n_loci];
}

int64_t sko_pileup_reads_mapq(const sko_read_batch* b, const sko_pileup_options* o, int mode, int64_t* call_off,
                              uint16_t* calls, int64_t capacity, uint32_t* spandel_count, uint32_t* submapped_count,
                              uint32_t* mapq_count, uint32_t* mapq_zero_count, uint64_t* mapq_sum_square)
{
    return pileup_reads_impl(b, o, mode, call_off, calls, capacity, spandel_count, submapped_count, mapq_count, mapq_zero_count,
                             mapq_sum_square, NULL);
}

/* the raw tier1 column (mode 0) and, parallel to its calls, what updateSomaticScoringMetrics gets for each of them
 * (starling_pos_processor_base.cpp:1360: readPos = read_pos, readLength = read_size): read_pos | read_size << 16 */
int64_t sko_pileup_reads_readpos(const sko_read_batch* b, const sko_pileup_options* o, int64_t* call_off, uint16_t* calls,
                                 int64_t capacity, uint32_t* read_pos)
{
    return pileup_reads_impl(b, o, 0, call_off, calls, capacity, NULL, NULL, NULL, NULL, NULL, read_pos);
}

typedef struct pl_col32 {
    uint32_t* v;
    int32_t n, cap;
} pl_col32;
static int pl_push32(pl_col32* c, uint32_t x)
{
    if (c->n == c->cap) {
        const int32_t nc = c->cap ? 2 * c->cap : 16;
        uint32_t* nv = (uint32_t*)realloc(c->v, sizeof(uint32_t) * (size_t)nc);
        if (!nv) return 1;
        c->v = nv;
        c->cap = nc;
    }
    c->v[c->n++] = x;
    return 0;
}

typedef struct pl_col64 {
    uint64_t* v;
    int32_t n, cap;
} pl_col64;
static int pl_push64(pl_col64* c, uint64_t x)
{
    if (c->n == c->cap) {
        const int32_t nc = c->cap ? 2 * c->cap : 16;
        uint64_t* nv = (uint64_t*)realloc(c->v, sizeof(uint64_t) * (size_t)nc);
        if (!nv) return 1;
        c->v = nv;
        c->cap = nc;
    }
    c->v[c->n++] = x;
    return 0;
}

static int64_t pileup_reads_impl(const sko_read_batch* b, const sko_pileup_options* o, int mode, int64_t* call_off,
                                 uint16_t* calls, int64_t capacity, uint32_t* spandel_count, uint32_t* submapped_count,
                                 uint32_t* mapq_count, uint32_t* mapq_zero_count, uint64_t* mapq_sum_square, uint32_t* read_pos)
{
    const int32_t n_loci = o->report_end - o->report_begin;
    pl_col64* ev = g_evs_words ? (pl_col64*)calloc((size_t)(n_loci > 0 ? n_loci : 1), sizeof(pl_col64)) : NULL;
    pl_col* t1 = (pl_col*)calloc((size_t)(n_loci > 0 ? n_loci : 1), sizeof(pl_col));
    pl_col* t2 = (pl_col*)calloc((size_t)(n_loci > 0 ? n_loci : 1), sizeof(pl_col));
    pl_col32* rp1 = (pl_col32*)calloc((size_t)(n_loci > 0 ? n_loci : 1), sizeof(pl_col32));
    int* delta = NULL;
    unsigned char* is_mm = NULL;
    int64_t result = -1;
    int bad = 0;
    if (spandel_count) memset(spandel_count, 0, sizeof(uint32_t) * (size_t)n_loci);
    if (submapped_count) memset(submapped_count, 0, sizeof(uint32_t) * (size_t)n_loci);
    if (mapq_count) memset(mapq_count, 0, sizeof(uint32_t) * (size_t)n_loci);
    if (mapq_zero_count) memset(mapq_zero_count, 0, sizeof(uint32_t) * (size_t)n_loci);
    if (mapq_sum_square) memset(mapq_sum_square, 0, sizeof(uint64_t) * (size_t)n_loci);

    for (int32_t r = 0; r < b->n_reads && !bad; ++r) { /* pileup_pos_reads: read after read, buffer order */
        const int64_t ro = b->read_off[r];
        const int L = (int)(b->read_off[r + 1] - ro);
        const sko_path_seg* path = b->path + b->path_off[r];
        const int nseg = (int)(b->path_off[r + 1] - b->path_off[r]);
        const uint8_t* code = b->read_code + ro;
        const uint8_t* qual = b->read_qual + ro;
        const int pos = b->pos[r];
        const int fwd = b->is_fwd[r] != 0;
        if (nseg == 0) continue; /* best_al.empty() :1148-1165 */

        int ref_len = 0, plen = 0, first_match = nseg, last_match = nseg; /* get_match_edge_segments */
        for (int i = 0; i < nseg; ++i) {
            if (pl_seg_ref_len(path[i].type)) ref_len += (int)path[i].length;
            if (pl_seg_read_len(path[i].type)) plen += (int)path[i].length;
            if (pl_seg_match(path[i].type)) {
                if (first_match == nseg) first_match = i;
                last_match = i;
            }
        }
        if (plen != L) { bad = 1; break; }
        const unsigned mapq = b->mapq[r];
        const unsigned adj_mapq = mapq < 5 ? 5 : mapq;                         /* :1181-1184 */
        const int is_mapq_adjust = o->is_mapq_adjust && (adj_mapq <= 80);
        if (ref_len > L + o->largest_total_indel_ref_span_per_read) continue; /* :1186-1191 */
        if (pos >= o->report_end) continue;                                   /* :1194-1198 */
        if (pos + ref_len <= o->report_begin) continue;

        int amb = 0; /* getReadAmbiguousEndLength, bam_seq_read_util.cpp:29-54 */
        if (fwd) {
            int e = L;
            while (e > 0 && pl_code_char(code[e - 1]) == 'N') --e;
            amb = L - e;
        } else {
            int s = 0;
            while (s < L && pl_code_char(code[s]) == 'N') ++s;
            amb = s;
        }
        int read_begin = 0, read_end = L;
        if (amb > 0) {
            if (fwd) read_end -= amb;
            else read_begin += amb;
        }
        if (o->min_distance_from_read_edge > 0) { /* :1220-1233 */
            read_begin += o->min_distance_from_read_edge;
            if (o->min_distance_from_read_edge <= read_end) read_end -= o->min_distance_from_read_edge;
            else read_end = 0;
            if (read_end <= read_begin) continue;
        }
        const unsigned level = b->map_level[r];
        const int is_submapped = !(level == 1 || level == 2);
        const int is_tier1 = (level == 1);
        const int mdf = o->mismatch_density_flank_size > 0;
        const int fs = o->mismatch_density_flank_size, fs2 = 2 * fs;
        const int delta_size = ((1 + fs2 > L) ? 1 + fs2 : L) - fs2;

        if (!is_submapped && mdf) { /* create_mismatch_filter_map, starling_read_util.cpp:121-213 */
            delta = (int*)realloc(delta, sizeof(int) * (size_t)(delta_size + 1));
            is_mm = (unsigned char*)realloc(is_mm, (size_t)(L + 1));
            memset(delta, 0, sizeof(int) * (size_t)delta_size);
            memset(is_mm, 0, (size_t)L);
#define PL_INC(start, length)                                                                  \
    do {                                                                                       \
        delta[((fs2 > (start)) ? fs2 : (start)) - fs2] += 1;                                   \
        if (((start) + (length)) < delta_size) delta[(start) + (length)] -= 1;                 \
    } while (0)
            int read_head = 0, ref_head = pos;
            for (int i = 0; i < nseg; ++i) {
                const uint32_t t = path[i].type;
                const int len = (int)path[i].length;
                const int edge = (i < first_match) || (i > last_match);
                if (t == 2) {
                    if (!edge) PL_INC(read_head, len);
                    read_head += len;
                } else if (t == 3) {
                    if (!edge) PL_INC(read_head, 0);
                    ref_head += len;
                } else if (pl_seg_match(t)) {
                    for (int j = 0; j < len; ++j) {
                        const int rp = read_head + j;
                        if (rp < read_begin || rp >= read_end) continue;
                        const int refp = ref_head + j;
                        const char rc = pl_code_char(code[rp]);
                        if (rc != pl_ref_char(b, refp)) {
                            int cand = 0; /* CandidateSnvBuffer::isCandidateSnvAnySample */
                            if (b->cand_snv_mask && refp >= b->ref_offset && refp < b->ref_offset + b->ref_len) {
                                const int id = rc == 'A' ? 0 : rc == 'C' ? 1 : rc == 'G' ? 2 : rc == 'T' ? 3 : 4;
                                cand = id < 4 && ((b->cand_snv_mask[refp - b->ref_offset] >> id) & 1);
                            }
                            if (!cand) {
                                is_mm[rp] = 1;
                                PL_INC(rp, 1);
                            }
                        }
                    }
                    read_head += len;
                    ref_head += len;
                } else if (t == 5) {
                    read_head += len;
                } else if (t == 4) {
                    ref_head += len;
                }
            }
            for (int i = 1; i < delta_size; ++i) delta[i] += delta[i - 1]; /* ddata::total */
        }

        int read_head = 0, ref_head = pos;
        for (int i = 0; i < nseg && !bad; ++i) {
            const uint32_t t = path[i].type;
            const int len = (int)path[i].length;
            if (pl_seg_match(t)) {
                for (int j = 0; j < len; ++j) {
                    const int rp = read_head + j;
                    if (rp < read_begin || rp >= read_end) continue;
                    const int refp = ref_head + j;
                    if (refp < o->report_begin || refp >= o->report_end) continue; /* is_pos_reportable */
                    const int locus = refp - o->report_begin;
                    const uint8_t c = code[rp];
                    const unsigned id = c == 1 ? 0 : c == 2 ? 1 : c == 4 ? 2 : c == 8 ? 3 : 4; /* bam_seq_code_to_id */
                    int q = qual[rp];
                    if (is_mapq_adjust) q = sko_mapped_qscore(q, (int)adj_mapq);
                    int current = 1, tscf = 0, nmm = 0;
                    if (!is_submapped) {
                        int is_call_filter = (c == 15) || (q < o->min_basecall_qscore);
                        int is_t2 = is_call_filter;
                        if (mdf) {
                            const int idx0 = ((fs > rp) ? fs : rp) - fs;
                            const int del = delta[(idx0 < delta_size - 1) ? idx0 : delta_size - 1]; /* ddata::get */
                            if (!is_call_filter) {
                                is_call_filter = (o->mismatch_density_max_count < del);
                                is_t2 = o->use_tier2_evidence ? (o->tier2_mismatch_density_max_count < del) : is_call_filter;
                            }
                            nmm = (del - (int)is_mm[rp]) > 0;
                        }
                        current = is_tier1 ? is_call_filter : is_t2;
                        tscf = is_tier1 && is_call_filter && !is_t2;
                    }
                    if (mapq_count) mapq_count[locus]++; /* :1346, before the submapped test */
                    if (mapq_zero_count && mapq == 0) mapq_zero_count[locus]++;
                    if (mapq_sum_square) mapq_sum_square[locus] += (uint64_t)(mapq * mapq);
                    if (ev) { /* updateGermlineScoringMetrics :1348-1357 */
                        const unsigned cycle = fwd ? (unsigned)rp : (unsigned)(L - (rp + 1));
                        const unsigned edge = (unsigned)((rp < L - (rp + 1)) ? rp : L - (rp + 1));
                        /* (a submapped position only feeds the MAPQ rank sum: its other fields are left 0) */
                        const uint64_t w = is_submapped ? ((uint64_t)id | ((uint64_t)mapq << 3) | ((uint64_t)1 << 34))
                                                        : ((uint64_t)id | ((uint64_t)mapq << 3) | ((uint64_t)(unsigned)q << 11) |
                                                           ((uint64_t)cycle << 18) | ((uint64_t)(edge < 20 ? edge : 20) << 29));
                        if (pl_push64(&ev[locus], w)) bad = 1;
                    }
                    if (is_submapped) {
                        if (submapped_count) submapped_count[locus]++;
                        continue;
                    }
                    const unsigned qb = (unsigned)(q > 63 ? 63 : q); /* base_call ctor, snp_pos_info.hh:70 */
                    const uint16_t bc = (uint16_t)(qb | (id << 6) | ((unsigned)fwd << 10) | ((unsigned)nmm << 11) |
                                                   ((unsigned)current << 12) | ((unsigned)tscf << 13));
                    if (pl_push(is_tier1 ? &t1[locus] : &t2[locus], bc)) bad = 1;
                    if (read_pos && is_tier1 && pl_push32(&rp1[locus], (uint32_t)rp | ((uint32_t)L << 16))) bad = 1;
                }
            } else if (t == 3) {
                const int edge = (i < first_match) || (i > last_match);
                if (!edge) {
                    for (int j = 0; j < len; ++j) {
                        const int refp = ref_head + j;
                        if (refp < o->report_begin || refp >= o->report_end) continue;
                        uint32_t* ctr = is_submapped ? submapped_count : spandel_count;
                        if (ctr) ctr[refp - o->report_begin]++;
                    }
                }
            }
            if (pl_seg_read_len(t)) read_head += len;
            if (pl_seg_ref_len(t)) ref_head += len;
        }
    }

    if (!bad) {
        int64_t n = 0;
        for (int32_t l = 0; l < n_loci && !bad; ++l) {
            call_off[l] = n;
#define PL_OUT(x)                                  \
    do {                                           \
        if (n >= capacity) { bad = 1; break; }     \
        calls[n++] = (x);                          \
    } while (0)
            if (mode == 0) {
                for (int i = 0; i < t1[l].n && !bad; ++i) {
                    if (read_pos && n < capacity) read_pos[n] = rp1[l].v[i];
                    PL_OUT(t1[l].v[i]);
                }
            } else if (mode == 1) {
                for (int i = 0; i < t2[l].n && !bad; ++i) PL_OUT(t2[l].v[i]);
            } else { /* CleanPileupFilter, PileupCleaner.cpp:28-66 */
                const int inc2 = (mode == 3);
                for (int i = 0; i < t1[l].n && !bad; ++i) {
                    const uint16_t bc = t1[l].v[i];
                    if ((bc >> 12) & 1) {
                        if (!(inc2 && ((bc >> 13) & 1))) continue;
                    }
                    PL_OUT(bc);
                }
                if (inc2)
                    for (int i = 0; i < t2[l].n && !bad; ++i) {
                        if ((t2[l].v[i] >> 12) & 1) continue;
                        PL_OUT(t2[l].v[i]);
                    }
            }
        }
        if (!bad) {
            call_off[n_loci] = n;
            result = n;
        }
        if (!bad && ev) {
            int64_t m = 0;
            for (int32_t l = 0; l < n_loci && !bad; ++l) {
                g_evs_off[l] = m;
                for (int i = 0; i < ev[l].n; ++i) {
                    if (m >= g_evs_capacity) { bad = 1; result = -1; break; }
                    g_evs_words[m++] = ev[l].v[i];
                }
            }
            if (!bad) g_evs_off[n_loci] = m;
        }
    }
    if (ev) {
        for (int32_t l = 0; l < n_loci; ++l) free(ev[l].v);
        free(ev);
    }
    for (int32_t l = 0; l < n_loci; ++l) {
        free(t1[l].v);
        free(t2[l].v);
        free(rp1[l].v);
    }
    free(t1);
    free(t2);
    free(rp1);
    free(delta);
    free(is_mm);
    return result;
}

/* ------------------------------------------------------------------------------------- GlobalAligner<int> (next row, rank 2)
 * Restatement of GlobalAligner<ScoreType>::align (L/alignment/GlobalAlignerImpl.hh:35-228): affine-gap global alignment
 * of a query to a reference with match/delete/insert states, off-edge soft clipping, optional edge insertion / required
 * edge deletion; max3 tie order (L/alignment/AlignerBase.hh:75-95); start-point selection (updateBacktrace,
 * L/alignment/Alignment.hh); traceback and '='/'X' expansion (SingleRefAlignerSharedImpl.hh:96-195,
 * L/blt_util/align_path_impl.hh:36-86). */

static unsigned char ga_max3(int* mx, int v0, int v1, int v2)
{
    unsigned char ptr = 0;
    *mx = v0;
    if (v1 > v0) { *mx = v1; ptr = 1; }
    if (v2 > *mx) { *mx = v2; ptr = 2; }
    return ptr;
}

typedef struct ga_bt {
    int max, state, queryBegin, refBegin, isInit;
} ga_bt;
static void ga_update(int thisMax, int refIndex, int queryIndex, ga_bt* bt, int state)
{
    if (!bt->isInit || thisMax > bt->max) {
        bt->max = thisMax;
        bt->refBegin = refIndex;
        bt->queryBegin = queryIndex;
        bt->isInit = 1;
        bt->state = state;
    }
}

int sko_global_align(const char* query, int querySize, const char* ref, int refSize, const sko_align_scores* sc,
                     int32_t* out_score, int32_t* out_begin_pos, sko_path_seg* out_path, int path_cap)
{
    if (querySize <= 0 || refSize <= 0) return -1;
    enum { ST_MATCH = 0, ST_DELETE = 1, ST_INSERT = 2 };
    const int badVal = -10000;
    const size_t W = (size_t)refSize + 1;
    int* s1 = (int*)malloc(sizeof(int) * 3 * ((size_t)querySize + 1));
    int* s2 = (int*)malloc(sizeof(int) * 3 * ((size_t)querySize + 1));
    unsigned char* ptr = (unsigned char*)malloc(3 * ((size_t)querySize + 1) * W); /* [q][r][state] */
    if (!s1 || !s2 || !ptr) { free(s1); free(s2); free(ptr); return -1; }
#define PTR(q, r, s) ptr[(((size_t)(q)) * W + (size_t)(r)) * 3 + (s)]
    int* thisSV = s1;
    int* prevSV = s2;
    for (int q = 0; q <= querySize; ++q) {
        PTR(q, 0, ST_MATCH) = ST_MATCH;
        thisSV[3 * q + ST_MATCH] = q * sc->offEdge;
        PTR(q, 0, ST_DELETE) = ST_MATCH;
        thisSV[3 * q + ST_DELETE] = badVal;
        if (!sc->isAllowEdgeInsertion) {
            PTR(q, 0, ST_INSERT) = ST_MATCH;
            thisSV[3 * q + ST_INSERT] = badVal;
        } else {
            PTR(q, 0, ST_INSERT) = ST_INSERT;
            thisSV[3 * q + ST_INSERT] = sc->open + (q * sc->extend);
        }
    }
    ga_bt bt = { 0, ST_MATCH, 0, 0, 0 };
    for (int r = 0; r < refSize; ++r) {
        int* t = thisSV; thisSV = prevSV; prevSV = t;
        if (!sc->isRequireEdgeDeletion) {
            PTR(0, r + 1, ST_MATCH) = ST_MATCH;
            thisSV[ST_MATCH] = 0;
            PTR(0, r + 1, ST_DELETE) = ST_MATCH;
            thisSV[ST_DELETE] = badVal;
        } else {
            PTR(0, r + 1, ST_MATCH) = ST_MATCH;
            thisSV[ST_MATCH] = badVal;
            PTR(0, r + 1, ST_DELETE) = ST_DELETE;
            thisSV[ST_DELETE] = sc->open + ((r + 1) * sc->extend);
        }
        PTR(0, r + 1, ST_INSERT) = ST_MATCH;
        thisSV[ST_INSERT] = badVal;
        for (int q = 0; q < querySize; ++q) {
            int* head = thisSV + 3 * (q + 1);
            {
                const int* sv = prevSV + 3 * q;
                PTR(q + 1, r + 1, ST_MATCH) = ga_max3(&head[ST_MATCH], sv[ST_MATCH], sv[ST_DELETE], sv[ST_INSERT]);
                head[ST_MATCH] += (query[q] == ref[r]) ? sc->match : sc->mismatch;
            }
            {
                const int* sv = prevSV + 3 * (q + 1);
                PTR(q + 1, r + 1, ST_DELETE) = ga_max3(&head[ST_DELETE], sv[ST_MATCH] + sc->open, sv[ST_DELETE], sv[ST_INSERT] + sc->insertDelete);
                head[ST_DELETE] += sc->extend;
                if (r == 0) head[ST_DELETE] = badVal;
            }
            {
                const int* sv = thisSV + 3 * q;
                PTR(q + 1, r + 1, ST_INSERT) = ga_max3(&head[ST_INSERT], sv[ST_MATCH] + sc->open, badVal, sv[ST_INSERT]);
                head[ST_INSERT] += sc->extend;
                if (q == 0) head[ST_INSERT] = badVal;
            }
        }
        if (!sc->isRequireEdgeDeletion) ga_update(thisSV[3 * querySize + ST_MATCH], r + 1, querySize, &bt, ST_MATCH);
    }
    if (sc->isRequireEdgeDeletion) {
        ga_update(thisSV[3 * querySize + ST_MATCH], refSize, querySize, &bt, ST_MATCH);
        ga_update(thisSV[3 * querySize + ST_DELETE], refSize, querySize, &bt, ST_DELETE);
    }
    if (sc->isAllowEdgeInsertion) ga_update(thisSV[3 * querySize + ST_INSERT], refSize, querySize, &bt, ST_INSERT);
    for (int q = 0; q < querySize; ++q)
        ga_update(thisSV[3 * q + ST_MATCH] + (querySize - q) * sc->offEdge, refSize, q, &bt, ST_MATCH);

    /* backTraceAlignment: segments are collected in reverse */
    *out_score = bt.max;
    int nseg = 0, bad = 0;
    sko_path_seg* rev = (sko_path_seg*)malloc(sizeof(sko_path_seg) * ((size_t)querySize + (size_t)refSize + 4));
    uint32_t ps_type = 0 /* NONE */, ps_len = 0;
    if (bt.queryBegin < querySize) { ps_type = 5; /* SOFT_CLIP */ ps_len = (uint32_t)(querySize - bt.queryBegin); }
#define GA_UPDATE_PATH(atype)                                                       \
    do {                                                                            \
        if (ps_type != (atype)) {                                                   \
            if (ps_type != 0) { rev[nseg].type = ps_type; rev[nseg].length = ps_len; ++nseg; } \
            ps_type = (atype);                                                      \
            ps_len = 0;                                                             \
        }                                                                           \
    } while (0)
    for (;;) {
        const int next = PTR(bt.queryBegin, bt.refBegin, bt.state);
        if (bt.state == ST_MATCH) {
            if (bt.queryBegin < 1 || bt.refBegin < 1) break;
            GA_UPDATE_PATH(1u);
            bt.queryBegin--;
            bt.refBegin--;
        } else if (bt.state == ST_DELETE) {
            if (bt.refBegin < 1) break;
            GA_UPDATE_PATH(3u);
            bt.refBegin--;
        } else {
            if (bt.queryBegin < 1) break;
            GA_UPDATE_PATH(2u);
            bt.queryBegin--;
        }
        bt.state = next;
        ps_len++;
    }
    if (ps_type != 0) { rev[nseg].type = ps_type; rev[nseg].length = ps_len; ++nseg; }
    if (bt.queryBegin != 0) { rev[nseg].type = 5; rev[nseg].length = (uint32_t)bt.queryBegin; ++nseg; }
    *out_begin_pos = bt.refBegin;
    /* reverse + apath_add_seqmatch */
    int n_out = 0;
    int qi = 0, ri = bt.refBegin;
    for (int k = nseg - 1; k >= 0 && !bad; --k) {
        const uint32_t t = rev[k].type, len = rev[k].length;
        if (t == 1) {
            for (uint32_t j = 0; j < len; ++j) {
                int same = (query[qi] == ref[ri]);
                if (query[qi] == 'N' || ref[ri] == 'N') same = 0;
                const uint32_t st = same ? 8u : 9u; /* SEQ_MATCH / SEQ_MISMATCH */
                if (n_out > 0 && out_path[n_out - 1].type == st) out_path[n_out - 1].length++;
                else {
                    if (n_out >= path_cap) { bad = 1; break; }
                    out_path[n_out].type = st;
                    out_path[n_out].length = 1;
                    ++n_out;
                }
                ++qi;
                ++ri;
            }
        } else {
            if (n_out >= path_cap) { bad = 1; break; }
            out_path[n_out].type = t;
            out_path[n_out].length = len;
            ++n_out;
            if (t == 2 || t == 5) qi += (int)len;
            if (t == 3) ri += (int)len;
        }
    }
    free(rev);
    free(s1);
    free(s2);
    free(ptr);
    return bad ? -1 : n_out;
}
