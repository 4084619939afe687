// The host bookkeeping shared by everything that reads x between two steps of the device time loop (time_loop.hip:
// after_step / work_due_after_next): the statistics, the probe records and the monitor records.  Plain C++17, no HIP:
// tests/record_log_main.cpp drives it alone.
//
//   StepCadence  counts the steps and says at which of them work is due.  tick() and due_after_next() ask ONE question
//                (due) of `count` and of `count + 1`, so that a two-step graph is split at exactly the step where the
//                work then happens.
//   RecordIndex  hands out the rows of a log of `capacity` records.  A full log drops: claim() returns -1, counts the
//                drop and the caller does no device work; nothing is overwritten.  reset() restarts the log; the step
//                counter lives in the cadence and goes on.
#ifndef TPSRHS_RECORD_LOG_HPP_
#define TPSRHS_RECORD_LOG_HPP_

#include <cstdint>
#include <vector>

namespace tpsrhs {

struct StepCadence {
  int64_t interval = 0;  // 0: off, never due
  int64_t start = 0;     // no work before this step
  int64_t count = 0;     // steps taken
  bool due(int64_t c) const { return interval > 0 && c % interval == 0 && c >= start; }
  // one more step is taken: is work due after it?
  bool tick() { return due(++count); }
  // would tick() say yes at the next step?
  bool due_after_next() const { return due(count + 1); }
};

struct RecordIndex {
  int64_t capacity = 0;
  int64_t nrecords = 0, ndropped = 0;
  std::vector<int64_t> iters;  // [nrecords] the step count at each record: the host issues every step and knows it
  // the row of the record taken at step `count`, or -1 (one more dropped record) when the log is full
  int64_t claim(int64_t count) {
    if (nrecords >= capacity) {
      ndropped++;
      return -1;
    }
    iters.push_back(count);
    return nrecords++;
  }
  void reset() {
    nrecords = ndropped = 0;
    iters.clear();
  }
};

}  // namespace tpsrhs
#endif
