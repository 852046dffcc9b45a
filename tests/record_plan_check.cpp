// The host side of the loop's recorder (csrc/pnmol_record_plan.hpp) on its own: built with -fsanitize=address,undefined and run by
// tests/test_record_host.py.  Checks the step -> slot mapping over split calls and a runt last step, the cursor, every refusal of
// the validation and of a call; exits non-zero on the first violation.
#include <cstdio>
#include <cstdlib>

#include "pnmol_record_plan.hpp"

namespace {

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s: line %d: %s\n", g_case, __LINE__, #cond);        \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)
const char* g_case = "";

bool contains(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// stand-ins for states and filters: only their addresses matter
struct Fixture {
    std::vector<int> storage;
    std::vector<const void*> slots, owners;
    int filter = 0, other_filter = 0, stepping = 0;
    explicit Fixture(int count) : storage((size_t)count) {
        for (int i = 0; i < count; ++i) slots.push_back(&storage[(size_t)i]), owners.push_back(&filter);
    }
    std::string validate(bool fp32 = false, bool running = false) const {
        return record_plan_validate((int)slots.size(), slots.data(), owners.data(), &filter, fp32, running);
    }
    RecordPlan plan() const {
        REQUIRE(validate().empty());
        RecordPlan p;
        record_plan_fill(&p, (int)slots.size(), slots.data());
        return p;
    }
};

void check_validation() {
    g_case = "validation";
    Fixture fx(5);
    REQUIRE(fx.validate().empty());
    REQUIRE(contains(fx.validate(true), "fp32"));
    REQUIRE(contains(fx.validate(false, true), "between pnmol_filter_steps_begin"));
    {
        Fixture bad(5);
        bad.slots[3] = nullptr;
        REQUIRE(contains(bad.validate(), "slot 3 is null"));
    }
    {
        Fixture bad(5);
        bad.owners[2] = &bad.other_filter;
        REQUIRE(contains(bad.validate(), "slot 2 is a state of another filter"));
    }
    {
        Fixture bad(5);
        bad.slots[4] = bad.slots[1];
        REQUIRE(contains(bad.validate(), "slot 4 is the state of slot 1 again"));
    }
    {
        Fixture bad(2);  // (the null slot is named although a duplicate follows; no owner is read for it)
        bad.slots[0] = nullptr, bad.slots[1] = nullptr;
        REQUIRE(contains(bad.validate(), "slot 0 is null"));
    }
    // clearing: any of count < 1 / no list; refused only inside a call, and never because of fp32
    REQUIRE(record_plan_validate(0, fx.slots.data(), fx.owners.data(), &fx.filter, true, false).empty());
    REQUIRE(record_plan_validate(5, nullptr, nullptr, &fx.filter, true, false).empty());
    REQUIRE(record_plan_validate(-3, nullptr, nullptr, &fx.filter, false, false).empty());
    REQUIRE(contains(record_plan_validate(0, nullptr, nullptr, &fx.filter, false, true), "between"));
    RecordPlan p = fx.plan();
    REQUIRE(p.set() && p.count == 5 && p.next == 0 && p.left() == 5);
    record_plan_fill(&p, 0, nullptr);
    REQUIRE(!p.set() && p.count == 0 && p.next == 0 && p.slots.empty() && !p.holds(fx.slots[0]));
    REQUIRE(record_plan_begin(p, 1000, &fx.stepping).empty());  // no recorder: nothing to refuse
}

// 13 steps in calls of 10 + 2 + 1 (the runt last step is a call of its own: another dt), as solve_on_device issues them
void check_mapping() {
    g_case = "mapping";
    Fixture fx(13);
    RecordPlan p = fx.plan();
    int filled = 0;
    for (int k : {10, 2, 1}) {
        REQUIRE(record_plan_begin(p, k, &fx.stepping).empty());
        for (int j = 0; j < k; ++j) {
            REQUIRE(record_plan_slot(p, j) == filled + j);
            REQUIRE(p.slots[(size_t)record_plan_slot(p, j)] == fx.slots[(size_t)(filled + j)]);
        }
        record_plan_advance(&p, k);
        filled += k;
        REQUIRE(p.next == filled && p.left() == 13 - filled);
    }
    REQUIRE(p.left() == 0);
    REQUIRE(contains(record_plan_begin(p, 1, &fx.stepping), "1 step(s) asked for, 0 of 13 recorder slot(s) left"));
    record_plan_advance(&p, 4);  // never past the end
    REQUIRE(p.next == 13);
    record_plan_advance(&p, -2);
    REQUIRE(p.next == 13);
}

void check_call_refusals() {
    g_case = "call refusals";
    Fixture fx(6);
    RecordPlan p = fx.plan();
    REQUIRE(record_plan_begin(p, 6, &fx.stepping).empty());
    REQUIRE(contains(record_plan_begin(p, 7, &fx.stepping), "7 step(s) asked for, 6 of 6"));
    record_plan_advance(&p, 4);
    REQUIRE(record_plan_begin(p, 2, &fx.stepping).empty());
    REQUIRE(contains(record_plan_begin(p, 3, &fx.stepping), "3 step(s) asked for, 2 of 6"));
    // the stepping state may be no slot at all: filled ones and ones to come alike
    for (int i = 0; i < 6; ++i) {
        REQUIRE(p.holds(fx.slots[(size_t)i]));
        REQUIRE(contains(record_plan_begin(p, 1, fx.slots[(size_t)i]), "one of the recorder's slots"));
    }
    REQUIRE(!p.holds(&fx.stepping) && !p.holds(nullptr));
    // a refused call leaves the plan as it was
    REQUIRE(p.next == 4 && p.count == 6);
}

}  // namespace

int main() {
    check_validation();
    check_mapping();
    check_call_refusals();
    std::puts("record plan: ok");
    return 0;
}
