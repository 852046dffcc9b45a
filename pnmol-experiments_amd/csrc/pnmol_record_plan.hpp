// pnmol_record_plan.hpp -- host side of the recorder of the constant-step loop (pnmol_filter_set_recorder, pnmol_record.hip):
// validation of a slot list, the refusals of one pnmol_filter_steps_begin call, the step -> slot mapping and the cursor.  Nothing
// of HIP in here and no state is dereferenced (slots and their owning filters come in as plain pointers):
// tests/record_plan_check.cpp builds it on its own under the sanitizers.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

struct RecordPlan {
    int count = 0;                    // slots
    int next = 0;                     // cursor: the slot the next step taken is recorded into
    std::vector<const void*> slots;   // the states, in the order they are filled
    std::vector<const void*> sorted;  // the same pointers sorted (membership tests)
    bool set() const { return count > 0; }
    int left() const { return count - next; }
    bool holds(const void* state) const { return std::binary_search(sorted.begin(), sorted.end(), state); }
};

// "" or why the arguments of pnmol_filter_set_recorder are refused.  owners[i]: the filter slots[i] belongs to (anything for a
// null slot); fp32 / call_running: what the filter says of itself.  count < 1 or no list: clears (refused only inside a call).
inline std::string record_plan_validate(int count, const void* const* slots, const void* const* owners, const void* filter,
                                        bool fp32, bool call_running) {
    if (call_running) return "called between pnmol_filter_steps_begin and pnmol_filter_steps_end";
    if (count < 1 || !slots) return "";
    if (fp32) return "an fp32 filter keeps no fp64 covariance to record";
    for (int i = 0; i < count; ++i) {
        if (!slots[i]) return "slot " + std::to_string(i) + " is null";
        if (!owners || owners[i] != filter) return "slot " + std::to_string(i) + " is a state of another filter";
    }
    std::vector<const void*> s(slots, slots + count);
    std::sort(s.begin(), s.end());
    const auto dup = std::adjacent_find(s.begin(), s.end());
    if (dup != s.end()) {
        const int first = (int)(std::find(slots, slots + count, *dup) - slots);
        const int second = (int)(std::find(slots + first + 1, slots + count, *dup) - slots);
        return "slot " + std::to_string(second) + " is the state of slot " + std::to_string(first) + " again";
    }
    return "";
}

// the plan from validated arguments; the cursor goes to slot 0
inline void record_plan_fill(RecordPlan* p, int count, const void* const* slots) {
    *p = RecordPlan{};
    if (count < 1 || !slots) return;
    p->count = count;
    p->slots.assign(slots, slots + count);
    p->sorted = p->slots;
    std::sort(p->sorted.begin(), p->sorted.end());
}

// "" or why a call of k steps that advances `stepping` in place is refused.  Touches nothing of the plan.
inline std::string record_plan_begin(const RecordPlan& p, int k, const void* stepping) {
    if (!p.set()) return "";
    if (k > p.left())
        return std::to_string(k) + " step(s) asked for, " + std::to_string(p.left()) + " of " + std::to_string(p.count) +
               " recorder slot(s) left";
    if (p.holds(stepping)) return "the state that is stepped is one of the recorder's slots";
    return "";
}

// the slot behind step j of the running call
inline int record_plan_slot(const RecordPlan& p, int j) { return p.next + j; }

// a call of k steps has been collected: its slots are filled (or, after a failing step, spent)
inline void record_plan_advance(RecordPlan* p, int k) { p->next = std::min(p->count, p->next + std::max(k, 0)); }
