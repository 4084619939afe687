// Stand-alone driver of tps_amd/csrc/record_log.hpp (tests/test_record_log.py builds it with plain g++, once without and once
// with -fsanitize=address,undefined, and runs it as a child process): the step cadence and the record index that the
// statistics, the probes and the monitor of the device time loop share.  For every (interval, start, capacity) it takes
// STEPS steps the way the loop does -- due_after_next() is asked before the step, tick() after it, a due step claims a row
// -- restarts the log after step RESET_AFTER (what *_read with reset does) and assigns the step counter after step
// SET_AFTER (what tpsrhs_stats_set_iter does), and prints one line per step.  The expected lines are recomputed in Python.
#include <cstdio>

#include "../tps_amd/csrc/record_log.hpp"

namespace {
constexpr int STEPS = 40, RESET_AFTER = 17, SET_AFTER = 29;
constexpr long long SET_COUNT = 8;

void print_iters(const char *what, const tpsrhs::RecordIndex &ix) {
  std::printf("%s nrecords %lld ndropped %lld iters", what, static_cast<long long>(ix.nrecords), static_cast<long long>(ix.ndropped));
  for (int64_t c : ix.iters) std::printf(" %lld", static_cast<long long>(c));
  std::printf("\n");
}

int run(int64_t interval, int64_t start, int64_t capacity) {
  std::printf("case interval %lld start %lld capacity %lld\n", static_cast<long long>(interval), static_cast<long long>(start),
              static_cast<long long>(capacity));
  tpsrhs::StepCadence cadence;
  cadence.interval = interval;
  cadence.start = start;
  tpsrhs::RecordIndex index;
  index.capacity = capacity;
  for (int step = 1; step <= STEPS; step++) {
    const bool due_next = cadence.due_after_next();
    const bool due = cadence.tick();
    char row[24] = ".";
    if (due) {
      const int64_t r = index.claim(cadence.count);
      if (r >= capacity || r < -1) return 1;  // a row outside the log: what a caller would write out of bounds
      std::snprintf(row, sizeof row, "%lld", static_cast<long long>(r));
    }
    std::printf("step %d count %lld due_next %d tick %d row %s nrecords %lld ndropped %lld\n", step,
                static_cast<long long>(cadence.count), due_next ? 1 : 0, due ? 1 : 0, row, static_cast<long long>(index.nrecords),
                static_cast<long long>(index.ndropped));
    if (index.iters.size() != static_cast<size_t>(index.nrecords)) return 1;
    if (step == RESET_AFTER) {
      print_iters("reset", index);
      index.reset();
    }
    if (step == SET_AFTER) cadence.count = SET_COUNT;
  }
  print_iters("end", index);
  return 0;
}
}  // namespace

int main() {
  const int64_t intervals[] = {1, 2, 3, 5}, starts[] = {0, 4}, capacities[] = {1, 3};
  for (int64_t interval : intervals)
    for (int64_t start : starts)
      for (int64_t capacity : capacities)
        if (run(interval, start, capacity) != 0) {
          std::printf("RECORD_LOG BROKEN\n");
          return 1;
        }
  // off: an interval of 0 is never due, whatever the counter says
  tpsrhs::StepCadence off;
  for (int step = 0; step < 3; step++)
    if (off.due_after_next() || off.tick()) {
      std::printf("RECORD_LOG BROKEN\n");
      return 1;
    }
  std::printf("RECORD_LOG DONE\n");
  return 0;
}
