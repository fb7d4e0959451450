// The control logic of plslam_lba_plan_optimize_dev (plslam_amd/csrc/lba_lm_ctl.hpp) on the CPU: g++ alone, no HIP header, no library.
//   test_lba_lm_ctl               the hand cases: one "PASS name" / "FAIL name: why" line each
//   test_lba_lm_ctl <case.txt>    replays one recorded run of the reference (tests/test_lba_lm_ctl_cpu.py writes the file from the
//                                 golden fixtures): lambda_lm lambda_k max_iters min_error_change min_error n_lm hmax n, then n
//                                 builds of err_raw dp_sumsq dx_sumsq_landmarks n_bad_pivots.  The builds are consumed in the order
//                                 the device's kernels call the functions, for as long as the stop word says "running":
//                                 "B lambda err applied" per build consumed, then "R iters n_builds stop lambda err err_prev".
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "lba_lm_ctl.hpp"

using namespace plslam;

struct Build { double err_raw, dp_ss, dx_ss; int n_bad; };
struct Rec { double lambda, err; int applied; };

// one pass as lba_lm_dev.hip runs it: K98 (first pass) | K99's prologue, solve and epilogue | K102
static void pass(LbaLmCtl& c, const LbaLmPrm& p, double hmax, const Build& b, std::vector<Rec>& tr)
{
    if (c.stop != LM_RUNNING) return;                  // every kernel of a pass: behind the stop word
    if (c.n_builds == 0) lm_on_hmax(c, p, hmax);
    const bool go = lm_on_err(c, p, b.err_raw);
    tr.push_back({go ? c.lambda : 0.0, c.err, c.apply});
    if (!go) return;
    lm_on_pivots(c, b.n_bad);
    c.dp_sumsq = b.dp_ss;
    tr.back().applied = c.apply;
    if (c.stop != LM_RUNNING) return;
    lm_on_step(c, p, b.dx_ss);
}

static int replay(const char* path)
{
    FILE* f = std::fopen(path, "r");
    if (!f) { std::perror(path); return 2; }
    LbaLmPrm p{};
    double hmax = 0;
    int n = 0;
    if (std::fscanf(f, "%lf %lf %d %lf %lf %lf %lf %d", &p.lambda_lm, &p.lambda_k, &p.max_iters, &p.min_error_change, &p.min_error, &p.n_lm,
                    &hmax, &n) != 8 || n < 0) { std::fclose(f); return 2; }
    std::vector<Build> builds((size_t)n);
    for (Build& b : builds)
        if (std::fscanf(f, "%lf %lf %lf %d", &b.err_raw, &b.dp_ss, &b.dx_ss, &b.n_bad) != 4) { std::fclose(f); return 2; }
    std::fclose(f);
    LbaLmCtl c;
    lm_init(c);
    std::vector<Rec> tr;
    for (const Build& b : builds) pass(c, p, hmax, b, tr);
    for (const Rec& r : tr) std::printf("B %.17g %.17g %d\n", r.lambda, r.err, r.applied);
    std::printf("R %d %d %d %.17g %.17g %.17g\n", c.iters, c.n_builds, c.stop, c.lambda, c.err, c.err_prev);
    return 0;
}

static int failures = 0;
static void report(const char* name, bool ok, const std::string& why = "")
{
    if (ok) std::printf("PASS %s\n", name);
    else { std::printf("FAIL %s: %s\n", name, why.c_str()); ++failures; }
}

static LbaLmPrm prm(int max_iters) { return LbaLmPrm{1e-5, 10.0, 1e-7, 1e-7, 100.0, max_iters, 0}; }

int main(int argc, char** argv)
{
    if (argc == 2) return replay(argv[1]);
    const double inf = std::numeric_limits<double>::infinity();
    {   // the first pass: err over the counters that are never incremented, lambda0, the step applied, no ||DX|| test
        LbaLmCtl c; lm_init(c); std::vector<Rec> tr; const LbaLmPrm p = prm(15);
        pass(c, p, 2e6, {500.0, 0.0, 0.0, 0}, tr);
        report("first_pass", c.err == inf && c.err_prev == inf && c.lambda == 1e-5 * 2e6 && c.hmax == 2e6 && c.apply == 1 && c.iters == 1 && c.stop == LM_RUNNING &&
                                 tr.size() == 1 && tr[0].applied == 1);
        LbaLmCtl z; lm_init(z); tr.clear();
        pass(z, p, 2e6, {0.0, 1.0, 1.0, 0}, tr);       // a zero sum: 0 / 0
        report("first_pass_zero_sum_is_nan", std::isnan(z.err) && z.apply == 1 && z.iters == 1 && z.stop == LM_RUNNING);
    }
    {   // max_iters = 1 and 0: the first solve only, stop 0
        for (int mi : {1, 0}) {
            LbaLmCtl c; lm_init(c); std::vector<Rec> tr;
            pass(c, prm(mi), 1.0, {5.0, 1.0, 1.0, 0}, tr);
            pass(c, prm(mi), 1.0, {4.0, 1.0, 1.0, 0}, tr);
            report(mi ? "max_iters_1" : "max_iters_0", c.stop == PLSLAM_LBA_STOP_MAX_ITERS && c.iters == 1 && c.n_builds == 1 && tr.size() == 1);
        }
    }
    {   // lambda grows on an applied step, shrinks on a rejected one; err_prev = err after a rejected step too; then the :1775 stop
        LbaLmCtl c; lm_init(c); std::vector<Rec> tr; const LbaLmPrm p = prm(15);
        const double l0 = 1e-5 * 1e5, l1 = l0 * 10.0, l2 = l1 / 10.0;
        pass(c, p, 1e5, {1.0, 1.0, 1.0, 0}, tr);
        pass(c, p, 1e5, {300.0, 1.0, 1.0, 0}, tr);     // err 3 against inf: applied, lambda x 10
        const bool a = c.lambda == l1 && c.err_prev == 3.0 && c.iters == 2 && tr[1].applied == 1 && tr[1].lambda == l0;
        pass(c, p, 1e5, {310.0, 1.0, 1.0, 0}, tr);     // 3.1 > 3: rejected, lambda / 10
        const bool b = c.lambda == l2 && c.err_prev == 3.1 && c.iters == 3 && tr[2].applied == 0 && tr[2].lambda == l1;
        pass(c, p, 1e5, {310.0, 1.0, 1.0, 0}, tr);     // the same err again: the first test
        const bool d = c.stop == PLSLAM_LBA_STOP_ERR && c.iters == 3 && tr[3].applied == -1 && tr[3].lambda == 0.0 && c.lambda == l2 && c.err_prev == 3.1;
        pass(c, p, 1e5, {1.0, 1.0, 1.0, 0}, tr);       // behind the stop: nothing
        report("schedule_reject_then_stop", a && b && d && tr.size() == 4 && c.n_builds == 4);
    }
    {   // min_error_change = 0: the loop goes on behind a rejection -- the same err again is NOT above err_prev, the retry is applied
        // at lambda / k, and lambda grows again behind it; a second rejection and retry follow the same schedule
        LbaLmCtl c; lm_init(c); std::vector<Rec> tr; LbaLmPrm p = prm(15); p.min_error_change = 0.0;
        const double l0 = 1e-5 * 1e5, l1 = l0 * 10.0, l2 = l1 / 10.0, l3 = l2 * 10.0, l4 = l3 / 10.0, l5 = l4 * 10.0;
        pass(c, p, 1e5, {1.0, 1.0, 1.0, 0}, tr);
        pass(c, p, 1e5, {300.0, 1.0, 1.0, 0}, tr);     // applied, lambda x 10
        pass(c, p, 1e5, {310.0, 1.0, 1.0, 0}, tr);     // 3.1 > 3: rejected, lambda / 10
        const bool a = tr[2].applied == 0 && tr[2].lambda == l1 && c.lambda == l2 && c.err_prev == 3.1 && c.stop == LM_RUNNING;
        pass(c, p, 1e5, {310.0, 1.0, 1.0, 0}, tr);     // the same err: |0| < 0 is false, 3.1 > 3.1 is false -- applied at l2, lambda x 10
        const bool b = tr[3].applied == 1 && tr[3].lambda == l2 && c.lambda == l3 && c.err_prev == 3.1 && c.iters == 4 && c.stop == LM_RUNNING;
        pass(c, p, 1e5, {320.0, 1.0, 1.0, 0}, tr);     // rejected again
        pass(c, p, 1e5, {320.0, 1.0, 1.0, 0}, tr);     // ... and retried
        const bool d = tr[4].applied == 0 && tr[4].lambda == l3 && tr[5].applied == 1 && tr[5].lambda == l4 && c.lambda == l5 && c.iters == 6 &&
                       c.err_prev == 3.2 && c.stop == LM_RUNNING;
        pass(c, p, 1e5, {315.0, 1.0, 1.0, 0}, tr);     // a descent behind it: applied at l5
        report("schedule_reject_then_retry", a && b && d && tr[6].applied == 1 && tr[6].lambda == l5 && c.lambda == l5 * 10.0 && c.n_builds == 7);
    }
    {   // err < min_error
        LbaLmCtl c; lm_init(c); std::vector<Rec> tr; const LbaLmPrm p = prm(15);
        pass(c, p, 1.0, {1.0, 1.0, 1.0, 0}, tr);
        pass(c, p, 1.0, {1e-6, 1.0, 1.0, 0}, tr);      // 1e-8 < 1e-7
        report("min_error", c.stop == PLSLAM_LBA_STOP_ERR && c.iters == 1 && c.apply == -1);
    }
    {   // the ||DX|| test: over both parts, for a rejected step too, never on the first pass; err_prev and iters stay
        LbaLmCtl c; lm_init(c); std::vector<Rec> tr; const LbaLmPrm p = prm(15);
        pass(c, p, 1.0, {1.0, 0.0, 0.0, 0}, tr);       // a zero first step: no test
        const bool a = c.stop == LM_RUNNING && c.iters == 1;
        pass(c, p, 1.0, {300.0, 0.5e-14, 0.4e-14, 0}, tr);   // sqrt(0.9e-14) < 1e-7
        const bool b = c.stop == PLSLAM_LBA_STOP_DX && c.iters == 1 && c.err_prev == inf && c.lambda == 1e-5 * 10.0 && tr[1].applied == 1;
        LbaLmCtl r; lm_init(r); tr.clear();
        pass(r, p, 1.0, {1.0, 1.0, 1.0, 0}, tr);
        pass(r, p, 1.0, {300.0, 1.0, 1.0, 0}, tr);
        pass(r, p, 1.0, {400.0, 0.0, 0.9e-14, 0}, tr);       // rejected AND small
        const bool d = r.stop == PLSLAM_LBA_STOP_DX && tr[2].applied == 0 && r.lambda == 1e-5 && r.err_prev == 3.0 && r.iters == 2;
        LbaLmCtl q; lm_init(q); tr.clear();
        pass(q, p, 1.0, {1.0, 1.0, 1.0, 0}, tr);
        pass(q, p, 1.0, {300.0, 0.6e-14, 0.6e-14, 0}, tr);   // sqrt(1.2e-14) > 1e-7: each part alone would stop
        report("dx_test", a && b && d && q.stop == LM_RUNNING && q.iters == 2);
    }
    {   // a bad pivot: stop 3, the step not applied, lambda / err_prev / iters as before the solve -- on the first pass and later
        LbaLmCtl c; lm_init(c); std::vector<Rec> tr; const LbaLmPrm p = prm(15);
        pass(c, p, 1.0, {1.0, 1.0, 1.0, 2}, tr);
        const bool a = c.stop == PLSLAM_LBA_STOP_NOT_PD && c.apply == 0 && c.iters == 0 && c.n_bad_pivots == 2 && tr[0].applied == 0 && c.lambda == 1e-5;
        LbaLmCtl d; lm_init(d); tr.clear();
        pass(d, p, 1.0, {1.0, 1.0, 1.0, 0}, tr);
        pass(d, p, 1.0, {300.0, 1.0, 1.0, 1}, tr);
        report("not_positive_definite", a && d.stop == PLSLAM_LBA_STOP_NOT_PD && d.apply == 0 && d.iters == 1 && d.lambda == 1e-5 && d.err_prev == inf &&
                                            tr[1].applied == 0 && tr[1].lambda == 1e-5);
    }
    {   // the loop runs out
        LbaLmCtl c; lm_init(c); std::vector<Rec> tr; const LbaLmPrm p = prm(3);
        for (int i = 0; i < 5; ++i) pass(c, p, 1.0, {100.0 * (10 - i), 1.0, 1.0, 0}, tr);
        report("runs_out", c.stop == PLSLAM_LBA_STOP_MAX_ITERS && c.iters == 3 && c.n_builds == 3 && tr.size() == 3 && c.lambda == (1e-5 * 10.0) * 10.0);
    }
    return failures ? 1 : 0;
}
