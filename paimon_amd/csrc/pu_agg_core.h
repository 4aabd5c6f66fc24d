// Partial-update fold with aggregate functions inside sequence groups
// (PartialUpdateMergeFunction.java: add :149-202, updateWithSequenceGroup
// :217-281, isEmptySequenceGroup :283-297, retractWithSequenceGroup :299-377,
// initRow :379-387, getResult :389-397) and the literal FieldAggregators
// (aggregate/Field*Agg.java; aggReversed(acc, in) = agg(in, acc),
// FieldAggregator.java).
//
// Shared scalar core, like changelog_core.h / lookup_core.h: k_emit_pu_sga
// (kernels.hip) and the host entry pmh_debug_pu_agg_fold (plan.cpp) run
// exactly this code through a member accessor A:
//   bool    A::valid(int x, int c)   member x's field c is non-null
//   int64_t A::load(int x, int c)    its stored element, sign-extended
// x indexes one key group's members in ascending (seq, isAdd) order, at most
// PAC_MAX_MEMBERS of them: the masks below are 32 bits wide and bit 31 is
// live, so nothing here shifts by the member count.
//
// The reference's sequential per-key state machine splits per sequence
// group: a group's fields depend only on the members' tuples of that group,
// so pac_scan_group resolves one group's order decisions in one walk (which
// members take part, which of them were in order AT THAT MOMENT, who holds
// the running tuple at the end) and pac_fold_col folds one aggregated column
// through them. No per-group table is kept anywhere.
#ifndef PMH_PU_AGG_CORE_H
#define PMH_PU_AGG_CORE_H

#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define PAC_HD __host__ __device__ inline
#else
#define PAC_HD inline
#endif

constexpr int PAC_MAX_MEMBERS = 32;

// aggregator codes (= PMH_AGG_*, kernels.h) and the ignore-retract wrapper
// bit; PAC_NONE marks a column without an aggregator
constexpr int PAC_LAST_NON_NULL = 0;
constexpr int PAC_LAST_VALUE = 1;
constexpr int PAC_FIRST_VALUE = 2;
constexpr int PAC_FIRST_NON_NULL = 3;
constexpr int PAC_SUM = 4;
constexpr int PAC_MAX = 5;
constexpr int PAC_MIN = 6;
constexpr int PAC_IGNORE_RETRACT = 0x80;
constexpr int PAC_NONE = 0xff;

// dtype codes (= PMH_DT_*, paimon_hip.h)
constexpr int PAC_DT_INT8 = 1;
constexpr int PAC_DT_INT16 = 2;
constexpr int PAC_DT_INT32 = 3;
constexpr int PAC_DT_INT64 = 4;
constexpr int PAC_DT_FLOAT32 = 5;
constexpr int PAC_DT_FLOAT64 = 6;

// how a member's field meets the accumulator
constexpr int PAC_MODE_AGG = 0;       // aggregator.agg(acc, in)
constexpr int PAC_MODE_REVERSED = 1;  // aggregator.aggReversed(acc, in)
constexpr int PAC_MODE_RETRACT = 2;   // aggregator.retract(acc, in)

// One field's fold state. bits: the stored element as 64 bits (sign-extended
// integers, raw float / double bits), 0 while null. init: the `initialized`
// member of FieldFirstValueAgg / FieldFirstNonNullValueAgg, reset per key.
// unsupported: a retract met an aggregator whose retract() throws.
struct PacState {
    int64_t bits;
    bool valid;
    bool init;
    bool unsupported;
};

// member kinds of one key group, 2 bits each (RowKind byte values)
PAC_HD int pac_kind(uint64_t kinds, int x) { return (int)((kinds >> (2 * x)) & 3); }
PAC_HD bool pac_is_retract(uint64_t kinds, int x) {
    return (pac_kind(kinds, x) & 1) != 0;  // UPDATE_BEFORE = 1, DELETE = 3
}

PAC_HD float pac_f32(int64_t b) {
    const uint32_t u = (uint32_t)b;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
PAC_HD int64_t pac_f32_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (int64_t)(int32_t)u;
}
PAC_HD double pac_f64(int64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}
PAC_HD int64_t pac_f64_bits(double d) {
    int64_t b;
    memcpy(&b, &d, 8);
    return b;
}

// IEEE total order on the stored bits (k_emit_agg's f32_ord / f64_ord)
PAC_HD uint64_t pac_ford(int64_t b, int dt) {
    if (dt == PAC_DT_FLOAT32) {
        const int32_t s = (int32_t)b;
        return s < 0 ? (uint64_t)(~(uint32_t)s)
                     : (uint64_t)((uint32_t)s | 0x80000000u);
    }
    return b < 0 ? ~(uint64_t)b : ((uint64_t)b | 0x8000000000000000ull);
}

// an integer sum back at the column width: two's complement wrap, then
// sign-extension (dtypes staged as 4-byte integers wrap at 32 bits)
PAC_HD int64_t pac_wrap(uint64_t u, int dt) {
    switch (dt) {
    case PAC_DT_INT8: return (int64_t)(int8_t)(uint8_t)u;
    case PAC_DT_INT16: return (int64_t)(int16_t)(uint16_t)u;
    case PAC_DT_INT64: return (int64_t)u;
    default: return (int64_t)(int32_t)(uint32_t)u;
    }
}

// a + sign * b in the column's arithmetic: unsigned for integers, so the
// wrap is defined; the column's own precision for float / double
PAC_HD int64_t pac_add(int64_t a, int64_t b, bool subtract, int dt) {
    if (dt == PAC_DT_FLOAT32)
        return pac_f32_bits(subtract ? pac_f32(a) - pac_f32(b)
                                     : pac_f32(a) + pac_f32(b));
    if (dt == PAC_DT_FLOAT64)
        return pac_f64_bits(subtract ? pac_f64(a) - pac_f64(b)
                                     : pac_f64(a) + pac_f64(b));
    const uint64_t ua = (uint64_t)a, ub = (uint64_t)b;
    return pac_wrap(subtract ? ua - ub : ua + ub, dt);
}
PAC_HD int64_t pac_negate(int64_t b, int dt) {
    if (dt == PAC_DT_FLOAT32) return pac_f32_bits(-pac_f32(b));
    if (dt == PAC_DT_FLOAT64) return pac_f64_bits(-pac_f64(b));
    return pac_wrap(0ull - (uint64_t)b, dt);
}

// aggregator.agg(a, b), literally: `a` stands where the reference has its
// accumulator parameter and `b` where it has inputField, whichever way
// round the caller passes them. *init is the aggregator's own flag.
PAC_HD void pac_agg(int agg, int dt, int64_t a_bits, bool a_ok, int64_t b_bits,
                    bool b_ok, bool *init, int64_t *r_bits, bool *r_ok) {
    bool take_b;
    switch (agg) {
    case PAC_LAST_VALUE: take_b = true; break;
    case PAC_LAST_NON_NULL: take_b = b_ok; break;
    case PAC_FIRST_VALUE:
        take_b = !*init;
        *init = true;
        break;
    case PAC_FIRST_NON_NULL:
        take_b = !*init && b_ok;
        if (take_b) *init = true;
        break;
    case PAC_SUM:
        if (a_ok && b_ok) {
            *r_bits = pac_add(a_bits, b_bits, false, dt);
            *r_ok = true;
            return;
        }
        take_b = !a_ok;
        break;
    default:  // PAC_MAX / PAC_MIN: compare(a, b) < 0 ? b : a (min: > 0)
        if (a_ok && b_ok) {
            bool lt, gt;
            if (dt == PAC_DT_FLOAT32 || dt == PAC_DT_FLOAT64) {
                const uint64_t oa = pac_ford(a_bits, dt);
                const uint64_t ob = pac_ford(b_bits, dt);
                lt = oa < ob;
                gt = oa > ob;
            } else {
                lt = a_bits < b_bits;
                gt = a_bits > b_bits;
            }
            take_b = agg == PAC_MAX ? lt : gt;
        } else {
            take_b = !a_ok;
        }
        break;
    }
    *r_bits = take_b ? (b_ok ? b_bits : 0) : (a_ok ? a_bits : 0);
    *r_ok = take_b ? b_ok : a_ok;
}

// One step of a field's fold: the member's field (in_bits, in_ok) meets the
// state through `mode`. agg_raw: aggregator code | PAC_IGNORE_RETRACT.
PAC_HD PacState pac_step(int agg_raw, int dt, PacState s, int64_t in_bits,
                         bool in_ok, int mode) {
    const int agg = agg_raw & 0x7f;
    if (!in_ok) in_bits = 0;
    if (mode == PAC_MODE_AGG) {
        pac_agg(agg, dt, s.bits, s.valid, in_bits, in_ok, &s.init, &s.bits,
                &s.valid);
        return s;
    }
    if (mode == PAC_MODE_REVERSED) {
        pac_agg(agg, dt, in_bits, in_ok, s.bits, s.valid, &s.init, &s.bits,
                &s.valid);
        return s;
    }
    // retract(acc, in)
    if (agg_raw & PAC_IGNORE_RETRACT) return s;  // FieldIgnoreRetractAgg
    switch (agg) {
    case PAC_LAST_VALUE:
        s.bits = 0;
        s.valid = false;
        break;
    case PAC_LAST_NON_NULL:
        if (in_ok) {
            s.bits = 0;
            s.valid = false;
        }
        break;
    case PAC_SUM:
        if (s.valid && in_ok) {
            s.bits = pac_add(s.bits, in_bits, true, dt);
        } else if (!s.valid) {  // negative(in); negative(null) is null
            s.bits = in_ok ? pac_negate(in_bits, dt) : 0;
            s.valid = in_ok;
        }
        break;
    default:  // FieldAggregator.retract throws
        s.unsupported = true;
        break;
    }
    return s;
}

// One sequence group's order decisions over a key group of gn members.
// fields[0..ns): the group's sequence-field columns.
//   *part  members that act on the group: a non-empty tuple, and not a
//          retract that ignore_delete swallows
//   *ord   those of them whose tuple was >= the row's running tuple at that
//          moment (lexicographic, nulls first, ties accept)
//   *cur   the member that holds the row's tuple at the end, -1 = none (the
//          row's sequence fields are null). A leading retract seeds it
//          (initRow), under ignore_delete too.
template <class A>
PAC_HD void pac_scan_group(const A &a, int gn, uint64_t kinds,
                           bool ignore_delete, const int16_t *fields, int ns,
                           uint32_t *part, uint32_t *ord, int *cur) {
    uint32_t p = 0, o = 0;
    int cu = pac_is_retract(kinds, 0) ? 0 : -1;
    for (int x = 0; x < gn; x++) {
        if (ignore_delete && pac_is_retract(kinds, x)) continue;
        bool anyv = false;
        for (int j = 0; j < ns; j++) anyv |= a.valid(x, fields[j]);
        if (!anyv) continue;  // isEmptySequenceGroup
        const uint32_t bit = (uint32_t)1 << x;
        p |= bit;
        int cmp = 0;
        for (int j = 0; j < ns && cmp == 0; j++) {
            const int c = fields[j];
            const bool va = a.valid(x, c);
            const bool vb = cu >= 0 && a.valid(cu, c);
            if (va != vb) {
                cmp = va ? 1 : -1;  // null sorts first
            } else if (va) {
                const int64_t ka = a.load(x, c);
                const int64_t kb = a.load(cu, c);
                if (ka != kb) cmp = ka > kb ? 1 : -1;
            }
        }
        if (cmp >= 0) {
            o |= bit;
            cu = x;
        }
    }
    *part = p;
    *ord = o;
    *cur = cu;
}

// Source member of a group's field WITHOUT an aggregator, -1 = null: the
// last in-order member sets it (an add even to null, a retract to null);
// with none in order the row keeps what initRow copied.
PAC_HD int pac_group_field_src(uint64_t kinds, uint32_t ord, int cur) {
    if (ord) return pac_is_retract(kinds, cur) ? -1 : cur;
    return pac_is_retract(kinds, 0) ? 0 : -1;
}

// An aggregated group field over the group's decisions. The accumulator
// starts null, or at the leading retract's field (initRow).
template <class A>
PAC_HD PacState pac_fold_col(const A &a, int gn, uint64_t kinds, uint32_t part,
                             uint32_t ord, int c, int agg_raw, int dt) {
    PacState s{0, false, false, false};
    if (pac_is_retract(kinds, 0)) {
        s.valid = a.valid(0, c);
        s.bits = s.valid ? a.load(0, c) : 0;
    }
    for (int x = 0; x < gn; x++) {
        if (!((part >> x) & 1)) continue;
        const bool iv = a.valid(x, c);
        const int64_t ib = iv ? a.load(x, c) : 0;
        const int mode = pac_is_retract(kinds, x) ? PAC_MODE_RETRACT
                         : ((ord >> x) & 1)       ? PAC_MODE_AGG
                                                  : PAC_MODE_REVERSED;
        s = pac_step(agg_raw, dt, s, ib, iv, mode);
    }
    return s;
}

// Source member of a field in no group, -1 = null: the last non-null among
// the add members (last_non_null_value is the only aggregator allowed there
// and equals this overlay), else what initRow copied. Retracts leave it.
template <class A>
PAC_HD int pac_plain_src(const A &a, int gn, uint64_t kinds, int c) {
    int src = pac_is_retract(kinds, 0) && a.valid(0, c) ? 0 : -1;
    for (int x = 0; x < gn; x++)
        if (!pac_is_retract(kinds, x) && a.valid(x, c)) src = x;
    return src;
}

// getResult's kind and sequence number: *has_add = some add member (else
// the result is a DELETE); *last = the last member ignore_delete did not
// swallow, -1 = none (latestSequenceNumber stays 0).
PAC_HD void pac_row_summary(int gn, uint64_t kinds, bool ignore_delete,
                            bool *has_add, int *last) {
    bool ha = false;
    int la = -1;
    for (int x = 0; x < gn; x++) {
        const bool rt = pac_is_retract(kinds, x);
        ha |= !rt;
        if (!(rt && ignore_delete)) la = x;
    }
    *has_add = ha;
    *last = la;
}

// The plan's tables the row fold reads. col_group[c]: group id or 0xff;
// sg_fields[g * 4 + j]: group g's sequence-field columns, sg_nseq[g] of them;
// grp_cols[grp_off[g] .. grp_off[g + 1]): group g's other fields;
// col_agg[c]: aggregator code | PAC_IGNORE_RETRACT, or PAC_NONE.
struct PacTables {
    int n_cols, n_groups;
    const uint8_t *col_dtype;
    const uint8_t *col_group;
    const int16_t *sg_fields;
    const uint8_t *sg_nseq;
    const int16_t *grp_cols;
    const uint16_t *grp_off;
    const uint8_t *col_agg;
};

// field c of member x (-1 = null) into the sink
template <class A, class S>
PAC_HD void pac_put_src(const A &a, S &sink, int c, int x) {
    const bool ok = x >= 0 && a.valid(x, c);
    sink.put(c, ok ? a.load(x, c) : 0, ok);
}

// One merged row of a key group with gn >= 2 members (singletons bypass the
// merge function): the sequence groups outermost, each group's sequence
// fields, then its other fields; the fields in no group last. The sink takes
// every column once through put(c, bits, ok), except those it claims with
// own(c) (the kernel's sequence-number and kind columns). Returns true when
// a retract met an aggregator without retract().
template <class A, class S>
PAC_HD bool pac_fold_row(const A &a, int gn, uint64_t kinds,
                         bool ignore_delete, const PacTables &t, S &sink) {
    bool bad = false;
    for (int g = 0; g < t.n_groups; g++) {
        const int16_t *fields = &t.sg_fields[g * 4];
        const int ns = t.sg_nseq[g];
        uint32_t part, ord;
        int cur;
        pac_scan_group(a, gn, kinds, ignore_delete, fields, ns, &part, &ord,
                       &cur);
        for (int j = 0; j < ns; j++) pac_put_src(a, sink, fields[j], cur);
        const int field_src = pac_group_field_src(kinds, ord, cur);
        for (int q = t.grp_off[g]; q < t.grp_off[g + 1]; q++) {
            const int c = t.grp_cols[q];
            const int ag = t.col_agg[c];
            if (ag == PAC_NONE) {
                pac_put_src(a, sink, c, field_src);
                continue;
            }
            const PacState s =
                pac_fold_col(a, gn, kinds, part, ord, c, ag, t.col_dtype[c]);
            bad |= s.unsupported;
            sink.put(c, s.valid ? s.bits : 0, s.valid);
        }
    }
    for (int c = 0; c < t.n_cols; c++) {
        if (t.col_group[c] != 0xff || sink.own(c)) continue;
        pac_put_src(a, sink, c, pac_plain_src(a, gn, kinds, c));
    }
    return bad;
}

// ------------------------------------------------------------- host entry
// One key group given as plain arrays (pmh_debug_pu_agg_fold's arguments,
// paimon_hip.h): what the CPU tests and pu_agg_hostcheck drive.
struct PacHostMembers {
    const int64_t *values;
    const uint8_t *valid_bytes;
    int n_cols;
    bool valid(int x, int c) const {
        return valid_bytes[(size_t)x * n_cols + c] != 0;
    }
    int64_t load(int x, int c) const { return values[(size_t)x * n_cols + c]; }
};

struct PacHostSink {
    int64_t *values;
    uint8_t *valid_bytes;
    bool own(int) const { return false; }
    void put(int c, int64_t bits, bool ok) {
        values[c] = bits;
        valid_bytes[c] = ok ? 1 : 0;
    }
};

// nullptr, or what is wrong with the arguments
inline const char *pac_host_check(int n_members, int n_cols, int n_groups,
                                  const uint8_t *col_group,
                                  const int16_t *sg_fields,
                                  const uint8_t *sg_nseq) {
    if (n_members < 1 || n_members > PAC_MAX_MEMBERS)
        return "n_members outside 1..32";
    if (n_cols < 1 || n_cols > 64) return "n_cols outside 1..64";
    if (n_groups < 0 || n_groups > 16) return "n_groups outside 0..16";
    for (int c = 0; c < n_cols; c++)
        if (col_group[c] != 0xff && col_group[c] >= n_groups)
            return "col_group names a group past n_groups";
    for (int g = 0; g < n_groups; g++) {
        if (sg_nseq[g] < 1 || sg_nseq[g] > 4)
            return "sg_nseq outside 1..4";
        for (int j = 0; j < sg_nseq[g]; j++) {
            const int c = sg_fields[g * 4 + j];
            if (c < 0 || c >= n_cols || col_group[c] != g)
                return "a sequence field is not a column of its group";
        }
    }
    return nullptr;
}

inline void pac_host_fold(int n_members, const int8_t *kinds, int n_cols,
                          const uint8_t *dtypes, const int64_t *values,
                          const uint8_t *valid, int n_groups,
                          const uint8_t *col_group, const int16_t *sg_fields,
                          const uint8_t *sg_nseq, const uint8_t *col_agg,
                          bool ignore_delete, int64_t *out_values,
                          uint8_t *out_valid, int32_t *out_kind,
                          int32_t *out_last, int32_t *out_unsupported) {
    const PacHostMembers a{values, valid, n_cols};
    PacHostSink sink{out_values, out_valid};
    uint64_t kw = 0;
    for (int x = 0; x < n_members; x++)
        kw |= (uint64_t)(kinds[x] & 3) << (2 * x);
    *out_unsupported = 0;
    if (n_members == 1) {  // ReducerMergeFunctionWrapper bypass
        for (int c = 0; c < n_cols; c++) pac_put_src(a, sink, c, 0);
        *out_kind = pac_kind(kw, 0);
        *out_last = 0;
        return;
    }
    // the per-group column lists, as the plan builds them
    std::vector<int16_t> gc;
    std::vector<uint16_t> go((size_t)n_groups + 1, 0);
    for (int g = 0; g < n_groups; g++) {
        for (int c = 0; c < n_cols; c++) {
            if (col_group[c] != g) continue;
            bool is_seq = false;
            for (int j = 0; j < sg_nseq[g]; j++)
                is_seq |= sg_fields[g * 4 + j] == c;
            if (!is_seq) gc.push_back((int16_t)c);
        }
        go[g + 1] = (uint16_t)gc.size();
    }
    const PacTables t{n_cols,  n_groups,  dtypes,    col_group, sg_fields,
                      sg_nseq, gc.data(), go.data(), col_agg};
    bool has_add;
    int last;
    pac_row_summary(n_members, kw, ignore_delete, &has_add, &last);
    *out_kind = has_add ? 0 : 3;
    *out_last = last;
    *out_unsupported =
        pac_fold_row(a, n_members, kw, ignore_delete, t, sink) ? 1 : 0;
}

#endif  // PMH_PU_AGG_CORE_H
