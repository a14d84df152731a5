// Timer.hpp -- hierarchical timers with the reference's surface (core/src/include/Timer.hpp:18-134,
// core/src/Timer.cpp:35-198): Timer::main.tick("name") descends into (or creates) a child node and starts
// it, tock() stops it and ascends; every node accumulates wall time, CPU time and an activation count;
// report() prints the tree with the share of the parent and the time per call.  ScopedTimer is the RAII
// form.  Two additions for a GPU step, independent of each other:
//  * tock() can first drain a HIP stream (setDeviceSync), so that the wall time of a node includes the device
//    work enqueued inside it -- without it the asynchronous launches would be charged to whichever node happens
//    to synchronise later.  That changes the run it measures: the host no longer runs ahead of the device.
//  * DEVICE-TIME nodes (setDeviceNode): children whose time was measured on the device with stream events
//    (the phase marks of include/nsdg.h), handed to the timer once, after the run -- never inside the step.  Such
//    a node prints in the same line format with "device time" where a host-clocked node says "wall time"; its
//    share of the parent is a ratio of DEVICE times: the parent's own device time (setDeviceTime on a host-clocked
//    parent such as `iterate`, whose wall-time line then shows what the host spent ENQUEUEING) or, for a
//    device-time parent, its device time.  An `overlapped` node (a ghost exchange on the communication stream)
//    ran beside its siblings: it is labelled so, gets no share, and belongs to no sum.
//
// In the reference the timers exist but no model code calls them; here Model and the
// model steps are instrumented; `model.timing = true` prints the report at the end of a run with a device
// synchronisation at every tock(), `model.phase_timing = true` prints it with the phase children of `iterate`
// and installs no synchronisation.
#pragma once
#include <chrono>
#include <ctime>
#include <functional>
#include <map>
#include <ostream>
#include <string>
#include <vector>

namespace Nextsim {

class Timer {
public:
    typedef std::string Key;
    Timer();
    explicit Timer(const Key& rootKey);

    void tick(const Key& timerName);
    void tock(const Key& timerName); //!< stops `timerName`, which must be the running node
    void tock();
    void reset();
    std::ostream& report(std::ostream& os) const;

    //! wall seconds / activation count of a node addressed by its path from the root, e.g. {"run", "iterate"}
    double wallSeconds(const std::vector<Key>& path) const;
    int ticks(const std::vector<Key>& path) const;

    //! path of the running node from the root (empty: the root itself), as wallSeconds() / setDeviceNode() take it
    std::vector<Key> currentPath() const;
    //! the device time of the node at `path`, which must exist: what the shares of its device-time children refer to
    void setDeviceTime(const std::vector<Key>& path, double seconds);
    //! creates or updates the device-time child `name` of the node at `path` (children keep the order of their first mention)
    void setDeviceNode(const std::vector<Key>& path, const Key& name, double seconds, int count, bool overlapped = false);
    //! device seconds of a node (-1: it has none)
    double deviceSeconds(const std::vector<Key>& path) const;

    //! called at every tock() before the clock is read (e.g. a stream synchronisation); may be empty
    void setDeviceSync(std::function<void()> sync) { m_sync = std::move(sync); }

    static Timer main;

private:
    struct Node {
        Key name;
        Node* parent = nullptr;
        std::map<Key, Node> children;
        std::vector<Key> order; // children in first-tick order
        double wall = 0, cpu = 0;
        double device = -1; // device seconds (stream events); < 0: none
        bool deviceNode = false, overlapped = false; // a node that has only a device time; one that ran beside its siblings
        int count = 0;
        bool running = false;
        std::chrono::steady_clock::time_point wall0;
        std::clock_t cpu0 = 0;
    };
    const Node* find(const std::vector<Key>& path) const;
    Node* find(const std::vector<Key>& path);
    static void print(std::ostream& os, const Node& n, const std::string& prefix, double parentWall, double parentDevice);
    Node root;
    Node* current;
    std::function<void()> m_sync;
};

//! RAII tick/tock on Timer::main (core/src/include/ScopedTimer.hpp)
class ScopedTimer {
public:
    explicit ScopedTimer(const Timer::Key& name) { Timer::main.tick(name); }
    ~ScopedTimer() { Timer::main.tock(); }
    ScopedTimer(const ScopedTimer&) = delete;
    ScopedTimer& operator=(const ScopedTimer&) = delete;
};

} // namespace Nextsim
