// The host side of the per-step tables of the constant-step loop (csrc/pnmol_cursor_plan.hpp) on its own: built with
// -fsanitize=address,undefined and run by tests/test_iterated_host.py.  Checks the step -> row mapping over split calls and a
// runt last step, the cursor after a failed call and a rehearsal, the refusal of a call in the words of every table, and what a set
// call does to the table it finds and to the captured graphs; exits non-zero on the first violation.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pnmol_cursor_plan.hpp"

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

CursorPlan plan_of(int count) {
    CursorPlan p;
    cursor_plan_fill(&p, count, true);
    return p;
}

void check_fill_and_no_table() {
    g_case = "fill, no table";
    CursorPlan p = plan_of(4);
    REQUIRE(p.set() && p.count == 4 && p.next == 0 && p.left() == 4);
    cursor_plan_collect(&p, 3, true);
    cursor_plan_fill(&p, 7, true);  // a table set again: the cursor goes to row 0
    REQUIRE(p.set() && p.count == 7 && p.next == 0);
    cursor_plan_fill(&p, 7, false);  // no table given: none set, whatever the count
    REQUIRE(!p.set() && p.count == 0 && p.next == 0);
    cursor_plan_fill(&p, 0, true);
    REQUIRE(!p.set() && p.count == 0 && p.next == 0);
    cursor_plan_fill(&p, -2, true);
    REQUIRE(!p.set() && p.count == 0 && p.next == 0);
    // no table: nothing is refused and collect is a no-op
    for (const LoopTableName& n : {LOOP_POINTS, LOOP_FORCING, LOOP_SCHEDULE}) REQUIRE(cursor_plan_begin(p, 1000, n.rows).empty());
    cursor_plan_collect(&p, 5, true);
    REQUIRE(p.next == 0 && p.count == 0);
    cursor_plan_rewind(&p, 3);
    REQUIRE(p.next == 0);
}

// 14 steps in calls of 13 + 1 (the runt last step is a call of its own: another dt), and in calls of 10 + 2 + 1 + 1
void check_mapping() {
    g_case = "mapping";
    for (const std::vector<int>& calls : {std::vector<int>{13, 1}, std::vector<int>{10, 2, 1, 1}}) {
        CursorPlan p = plan_of(14);
        int taken = 0;
        for (int k : calls) {
            REQUIRE(cursor_plan_begin(p, k, LOOP_FORCING.rows).empty());
            for (int j = 0; j < k; ++j) REQUIRE(cursor_plan_row(p, j) == taken + j);
            cursor_plan_collect(&p, k, true);
            taken += k;
            REQUIRE(p.next == taken && p.left() == 14 - taken);
        }
        REQUIRE(p.left() == 0);
        // the exact refusal, in the words of each table
        REQUIRE(cursor_plan_begin(p, 1, LOOP_POINTS.rows) == "1 step(s) asked for, 0 of 14 linearisation point(s) left");
        REQUIRE(cursor_plan_begin(p, 1, LOOP_FORCING.rows) == "1 step(s) asked for, 0 of 14 right-hand side(s) left");
        REQUIRE(cursor_plan_begin(p, 1, LOOP_SCHEDULE.rows) == "1 step(s) asked for, 0 of 14 row(s) of coefficients left");
        cursor_plan_collect(&p, 4, true);  // never past the end
        REQUIRE(p.next == 14);
        cursor_plan_collect(&p, -2, true);  // a negative k moves nothing
        REQUIRE(p.next == 14);
    }
    // what pnmol_filter_steps_begin's error calls each table
    REQUIRE(std::string(LOOP_POINTS.label) == "linearisation points" && std::string(LOOP_FORCING.label) == "forcing" &&
            std::string(LOOP_SCHEDULE.label) == "operator schedule");
}

void check_call_refusals_and_rewinding() {
    g_case = "call refusals, rewinding";
    CursorPlan p = plan_of(6);
    REQUIRE(cursor_plan_begin(p, 6, LOOP_POINTS.rows).empty());
    REQUIRE(contains(cursor_plan_begin(p, 7, LOOP_POINTS.rows), "7 step(s) asked for, 6 of 6"));
    cursor_plan_collect(&p, 4, true);
    REQUIRE(cursor_plan_begin(p, 2, LOOP_POINTS.rows).empty());
    REQUIRE(contains(cursor_plan_begin(p, 3, LOOP_POINTS.rows), "3 step(s) asked for, 2 of 6"));
    REQUIRE(p.next == 4 && p.count == 6);  // a refused call leaves the plan as it was
    // a call that failed consumes no row: the repeated call maps to the same rows
    cursor_plan_collect(&p, 2, false);
    REQUIRE(p.next == 4 && cursor_plan_row(p, 0) == 4 && cursor_plan_row(p, 1) == 5);
    cursor_plan_collect(&p, 3, false);
    REQUIRE(p.next == 4);
    cursor_plan_collect(&p, 2, true);
    REQUIRE(p.next == 6);
    // a rehearsal: the cursor is read, the call collected, the cursor put back; values outside the table are clamped
    cursor_plan_rewind(&p, 4);
    REQUIRE(p.next == 4 && p.left() == 2);
    cursor_plan_rewind(&p, -3);
    REQUIRE(p.next == 0);
    cursor_plan_rewind(&p, 99);
    REQUIRE(p.next == 6);
}

// what a set call does to the table it finds: {plan, cap, count, copy_ok} -> {replace, drop_graphs}
void check_set_calls() {
    g_case = "set calls";
    const CursorPlan unset, set8 = plan_of(8);
    struct Case {
        const char* what;
        CursorPlan plan;
        int cap, count;
        bool copy_ok, replace, drop_graphs;
    };
    const Case cases[] = {
        {"first set", unset, 0, 8, true, true, true},
        {"fits", set8, 8, 5, true, false, false},
        {"equal to cap", set8, 8, 8, true, false, false},
        {"one more than cap", set8, 8, 9, true, true, true},
        {"clear when set", set8, 8, 0, true, false, true},
        {"clear when unset", unset, 0, 0, true, false, false},
        {"failed copy in place", set8, 8, 5, false, false, true},
        // rows kept by a copy that failed are no table: the next set call goes from unset to set
        {"fits after a failed copy", unset, 8, 5, true, false, true},
        {"failed copy into fresh rows", set8, 8, 9, false, true, true},
        {"a table consumed to its end still fits", [] { CursorPlan p = plan_of(8); cursor_plan_collect(&p, 8, true); return p; }(), 8, 8,
         true, false, false},
    };
    for (const Case& c : cases) {
        g_case = c.what;
        const LoopTableChange ch = loop_table_change(c.plan, c.cap, c.count, c.copy_ok);
        REQUIRE(ch.replace == c.replace);
        REQUIRE(ch.drop_graphs == c.drop_graphs);
    }
    g_case = "set calls";
    REQUIRE(loop_table_change(set8, 8, 5).drop_graphs == false);  // (copy_ok defaults to true: the decision in front of the copy)
    LoopTable t;
    REQUIRE(!t.plan.set() && t.rows == nullptr && t.words == nullptr && t.cap == 0 && t.stride == 0);
}

}  // namespace

int main() {
    check_fill_and_no_table();
    check_mapping();
    check_call_refusals_and_rewinding();
    check_set_calls();
    std::puts("cursor plan: ok");
    return 0;
}
