"""Sequential, literal port of PartialUpdateMergeFunction with sequence
groups AND per-field aggregate functions (PartialUpdateMergeFunction.java:
add :149-202, updateWithSequenceGroup :217-281, isEmptySequenceGroup
:283-297, retractWithSequenceGroup :299-377, initRow, getResult :389-397,
getAggFuncName :698-728) and of the FieldAggregators it drives
(aggregate/Field*Agg.java), each with its `initialized` flag where it has
one, plus the ReducerMergeFunctionWrapper singleton bypass and drop-delete.

Ported by the letter, not by meaning: aggReversed(acc, in) IS agg(in, acc),
so first_value's reversed form returns the accumulator the first time and
the INPUT afterwards. Values are numpy scalars of the column's dtype, so
integer sums wrap at the column width and float sums round in the column's
precision, in member order.

pu_agg_model(runs, seq_groups, ...) returns the dict shape of
oracle.partial_update_seqgroup_model plus "counters" (what the stream
exercised; the GPU tests assert on them before they trust a seed).
"""
import numpy as np


class UnsupportedRetract(Exception):
    """FieldAggregator.retract's UnsupportedOperationException."""


class FieldAggregator:
    name = "?"

    def agg(self, acc, inp):
        raise NotImplementedError

    def agg_reversed(self, acc, inp):
        return self.agg(inp, acc)

    def reset(self):
        pass

    def retract(self, acc, inp):
        raise UnsupportedRetract(
            f"Aggregate function '{self.name}' does not support retraction,"
            " If you allow this function to ignore retraction messages,"
            " you can configure 'fields.${field_name}.ignore-retract'="
            "'true'.")


class LastValue(FieldAggregator):
    name = "last_value"

    def agg(self, acc, inp):
        return inp

    def retract(self, acc, inp):
        return None


class LastNonNullValue(FieldAggregator):
    name = "last_non_null_value"

    def agg(self, acc, inp):
        return acc if inp is None else inp

    def retract(self, acc, inp):
        return None if inp is not None else acc


class FirstValue(FieldAggregator):
    name = "first_value"

    def __init__(self):
        self.initialized = False

    def agg(self, acc, inp):
        if not self.initialized:
            self.initialized = True
            return inp
        return acc

    def reset(self):
        self.initialized = False


class FirstNonNullValue(FieldAggregator):
    name = "first_non_null_value"

    def __init__(self):
        self.initialized = False

    def agg(self, acc, inp):
        if not self.initialized and inp is not None:
            self.initialized = True
            return inp
        return acc

    def reset(self):
        self.initialized = False


class Sum(FieldAggregator):
    name = "sum"

    def agg(self, acc, inp):
        if acc is None or inp is None:
            return inp if acc is None else acc
        with np.errstate(over="ignore"):
            return acc + inp

    def retract(self, acc, inp):
        with np.errstate(over="ignore"):
            if acc is None or inp is None:
                if acc is None:
                    return None if inp is None else -inp
                return acc
            return acc - inp


def _compare(a, b):
    return -1 if a < b else (1 if a > b else 0)


class Max(FieldAggregator):
    name = "max"

    def agg(self, acc, inp):
        if acc is None or inp is None:
            return inp if acc is None else acc
        return inp if _compare(acc, inp) < 0 else acc


class Min(FieldAggregator):
    name = "min"

    def agg(self, acc, inp):
        if acc is None or inp is None:
            return inp if acc is None else acc
        return acc if _compare(acc, inp) < 0 else inp


class IgnoreRetract(FieldAggregator):
    def __init__(self, inner):
        self.inner = inner
        self.name = inner.name

    def agg(self, acc, inp):
        return self.inner.agg(acc, inp)

    def reset(self):
        self.inner.reset()

    def retract(self, acc, inp):
        return acc


AGGREGATORS = {
    "last_value": LastValue,
    "last_non_null_value": LastNonNullValue,
    "first_value": FirstValue,
    "first_non_null_value": FirstNonNullValue,
    "first_not_null_value": FirstNonNullValue,
    "sum": Sum,
    "max": Max,
    "min": Min,
}


def resolve_aggs(n_cols, seq_groups, aggs=None, ignore_retract=(),
                 default_agg=None):
    """getAggFuncName per value column -> {col: aggregator name}. A sequence
    field gets none; every function but last_non_null_value needs the column
    to be a group field."""
    aggs = dict(aggs or {})
    seq_fields = {c for sg in seq_groups for c in sg["sequence_fields"]}
    protected = {c for sg in seq_groups for c in sg["group_fields"]}
    out = {}
    for c in range(n_cols):
        if c in seq_fields:
            continue
        name = aggs.get(c, default_agg)
        if name is None:
            continue
        if name != "last_non_null_value" and c not in protected:
            raise ValueError("Must use sequence group for aggregation "
                             f"functions but not found for field {c}.")
        out[c] = name
    return out


def new_counters():
    return {"in_order": 0, "reversed": 0, "retract_in_order": 0,
            "retract_out_of_order": 0, "skipped_empty": 0,
            "largest_group": 0, "first_member_retract": 0}


def _tuple_ge(a, b):
    """FieldsComparator.compare(a, b) >= 0: lexicographic ascending, nulls
    FIRST."""
    for x, y in zip(a, b):
        if x is None and y is None:
            continue
        if x is None:
            return False
        if y is None:
            return True
        if x != y:
            return x > y
    return True


class PartialUpdateMerge:
    """The merge function over rows given as lists (None = null)."""

    def __init__(self, n_cols, seq_groups, agg_names=None, ignore_retract=(),
                 ignore_delete=False, counters=None):
        self.n_cols = n_cols
        self.ignore_delete = ignore_delete
        self.counters = counters if counters is not None else new_counters()
        # field index -> the compare fields of its group (fieldSeqComparators
        # holds one entry per sequence field AND per group field)
        self.comparators = {}
        for sg in seq_groups:
            fields = tuple(sg["sequence_fields"])
            for c in list(sg["sequence_fields"]) + list(sg["group_fields"]):
                self.comparators[c] = fields
        self.aggregators = {}
        ign = set(ignore_retract)
        for c, name in (agg_names or {}).items():
            a = AGGREGATORS[name]()
            self.aggregators[c] = IgnoreRetract(a) if c in ign else a
        self.reset()

    def reset(self):
        self.meet_insert = False
        self.filled = False  # notNullColumnFilled
        self.row = [None] * self.n_cols
        self.latest_seq = 0
        for a in self.aggregators.values():
            a.reset()

    def _is_empty_group(self, value, fields, processed):
        for f in fields:
            if value[f] is not None:
                return False
        for f in fields:
            processed[f] = True
        return True

    def add(self, kind, seq, value):
        if kind in (1, 3):
            if not self.filled:
                self.row = list(value)  # initRow
                self.filled = True
            if self.ignore_delete:
                return
            self.latest_seq = seq
            self._retract_with_sequence_group(value)
            return
        self.latest_seq = seq
        if not self.comparators:
            for i in range(self.n_cols):  # updateNonNullFields
                if value[i] is not None:
                    self.row[i] = value[i]
        else:
            self._update_with_sequence_group(value)
        self.meet_insert = True
        self.filled = True

    def _update_with_sequence_group(self, value):
        cnt = self.counters
        row = self.row
        processed = [False] * self.n_cols
        for i in range(self.n_cols):
            fields = self.comparators.get(i)
            aggregator = self.aggregators.get(i)
            acc = row[i]
            if fields is not None:
                if processed[i]:
                    continue
                first_of_group = i == min(
                    c for c, f in self.comparators.items() if f == fields)
                if self._is_empty_group(value, fields, processed):
                    if first_of_group:
                        cnt["skipped_empty"] += 1
                    continue
                field = value[i]
                if _tuple_ge([value[f] for f in fields],
                             [row[f] for f in fields]):
                    if i in fields:
                        for f in fields:
                            row[f] = value[f]
                            processed[f] = True
                        continue
                    if aggregator is None:
                        row[i] = field
                    else:
                        row[i] = aggregator.agg(acc, field)
                        cnt["in_order"] += 1
                elif aggregator is not None:
                    row[i] = aggregator.agg_reversed(acc, field)
                    cnt["reversed"] += 1
            else:
                field = value[i]
                if aggregator is not None:
                    row[i] = aggregator.agg(acc, field)
                elif field is not None:
                    row[i] = field

    def _retract_with_sequence_group(self, value):
        cnt = self.counters
        row = self.row
        updated = set()
        processed = [False] * self.n_cols
        for i in range(self.n_cols):
            fields = self.comparators.get(i)
            aggregator = self.aggregators.get(i)
            if fields is None:
                continue
            if processed[i]:
                continue
            first_of_group = i == min(
                c for c, f in self.comparators.items() if f == fields)
            if self._is_empty_group(value, fields, processed):
                if first_of_group:
                    cnt["skipped_empty"] += 1
                continue
            if _tuple_ge([value[f] for f in fields],
                         [row[f] for f in fields]):
                if i in fields:
                    for f in fields:
                        if f not in updated:
                            row[f] = value[f]
                            updated.add(f)
                        processed[f] = True
                elif aggregator is None:
                    row[i] = None  # retract normal field
                else:
                    row[i] = aggregator.retract(row[i], value[i])
                    cnt["retract_in_order"] += 1
            elif aggregator is not None:
                # retract agg field for old sequence
                row[i] = aggregator.retract(row[i], value[i])
                cnt["retract_out_of_order"] += 1

    def get_result(self):
        """-> (sequence number, kind, row)"""
        return self.latest_seq, (0 if self.meet_insert else 3), list(self.row)


def _sorted_stream(runs):
    key = np.concatenate([r["key"] for r in runs])
    seq = np.concatenate([r["seq"] for r in runs])
    kind = np.concatenate([r["kind"] for r in runs])
    run = np.concatenate([np.full(len(r["key"]), i, dtype=np.int32)
                          for i, r in enumerate(runs)])
    row = np.concatenate([np.arange(len(r["key"]), dtype=np.int64)
                          for r in runs])
    is_add = ((kind == 0) | (kind == 2)).astype(np.int8)
    order = np.lexsort((is_add, seq, key))
    return key[order], seq[order], kind[order], run[order], row[order]


def pu_agg_model(runs, seq_groups, aggs=None, ignore_retract=(),
                 default_agg=None, drop_delete=True, ignore_delete=False):
    """runs / seq_groups as oracle.partial_update_seqgroup_model takes them;
    aggs {col index: function name}; ignore_retract column indices;
    default_agg a function name or None. Raises UnsupportedRetract where the
    reference throws."""
    key, seq, kind, run, row = _sorted_stream(runs)
    n = len(key)
    n_cols = len(runs[0]["values"]) if runs else 0
    names = resolve_aggs(n_cols, seq_groups, aggs, ignore_retract,
                         default_agg)
    counters = new_counters()
    mf = PartialUpdateMerge(n_cols, seq_groups, names, ignore_retract,
                            ignore_delete, counters)

    def value_of(m):
        a, b = run[m], row[m]
        valid = runs[a].get("valid")
        return [None if valid is not None and not valid[c][b]
                else runs[a]["values"][c][b] for c in range(n_cols)]

    out = {"key": [], "seq": [], "kind": [],
           "values": [[] for _ in range(n_cols)],
           "valid": [[] for _ in range(n_cols)]}

    def emit(k, s, kd, vals):
        out["key"].append(k)
        out["seq"].append(s)
        out["kind"].append(kd)
        for c in range(n_cols):
            ok = vals[c] is not None
            out["values"][c].append(vals[c] if ok else 0)
            out["valid"][c].append(ok)

    i = 0
    while i < n:
        j = i
        while j + 1 < n and key[j + 1] == key[i]:
            j += 1
        gn = j - i + 1
        counters["largest_group"] = max(counters["largest_group"], gn)
        if gn == 1:  # ReducerMergeFunctionWrapper bypass
            if not (drop_delete and kind[i] in (1, 3)):
                emit(key[i], seq[i], int(kind[i]), value_of(i))
            i = j + 1
            continue
        if kind[i] in (1, 3):
            counters["first_member_retract"] += 1
        mf.reset()
        for m in range(i, j + 1):
            mf.add(int(kind[m]), seq[m], value_of(m))
        s, kd, vals = mf.get_result()
        if not (drop_delete and kd == 3):
            emit(key[i], s, kd, vals)
        i = j + 1
    return {
        "key": np.array(out["key"], np.int64),
        "seq": np.array(out["seq"], np.int64),
        "kind": np.array(out["kind"], np.int8),
        "values": [np.array(v, runs[0]["values"][c].dtype)
                   for c, v in enumerate(out["values"])],
        "valid": [np.array(v, bool) for v in out["valid"]],
        "counters": counters,
    }
