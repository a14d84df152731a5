#include "DynamicsOutputs.hpp"

#include <algorithm>
#include <limits>

#include "Rendezvous.hpp"
#include "Timer.hpp"

namespace Nextsim {

namespace {
void toHost(std::vector<double>& host, const double* device, const char* what)
{
    checkHip(hipMemcpy(host.data(), device, host.size() * sizeof(double), hipMemcpyDeviceToHost), what);
}
} // namespace

// ------------------------------------------------------------------------------------------------ history
void HistoryChannel::allocate(DynamicsBlock& b)
{ // the first sample of a window stores: no memset
    Part& p = m_parts[b.index];
    p.acc = b.outputBuffer(m_host.config().ids.size() * plane(b), "DynamicsStep: hipMalloc (history accumulator)");
    if (m_host.config().weighted())
        p.weight = b.outputBuffer(plane(b), "DynamicsStep: hipMalloc (history weights)");
}

void HistoryChannel::afterStep(long dt, const DynamicsBlocks& blocks)
{
    const HistoryOutput::Action a = m_host.step(dt);
    if (a.sample) {
        const HistoryOutput::Config& c = m_host.config();
        const std::vector<int>& ids = c.ids;
        const bool stats = c.hasStats(); // bare names: the plain call, as ever
        forEachBlock(blocks, [&](DynamicsBlock& b) {
            const nsdg_history_sources src = b.sources(m_state.thermodynamics, m_state.advectColumn);
            const Part& p = m_parts[b.index];
            if (stats)
                check(nsdg_history_accumulate_stats(b.ctx.get(), b.j0, b.j1, (int32_t)ids.size(), ids.data(), c.stats.data(), &src, a.store ? 1 : 0, b.j0,
                          (int64_t)plane(b), p.acc, p.weight),
                    "nsdg_history_accumulate_stats");
            else
                check(nsdg_history_accumulate(b.ctx.get(), b.j0, b.j1, (int32_t)ids.size(), ids.data(), &src, a.store ? 1 : 0, b.j0, (int64_t)plane(b), p.acc),
                    "nsdg_history_accumulate");
        });
    }
    if (a.flush)
        atStop(blocks);
}

void HistoryChannel::atStop(const DynamicsBlocks& blocks)
{
    // the window ends: the owned rows of every block of this process into ONE host array, divided by the count, one record file
    const long samples = m_host.samples();
    if (samples > 0) {
        ScopedTimer timer("history flush");
        const HistoryOutput::Config& c = m_host.config();
        const RowRange range(blocks);
        HistoryOutput::Record r;
        r.timeStart = m_host.windowStart(), r.timeEnd = m_host.windowEnd(), r.samples = samples;
        r.kind = c.snapshot ? "snapshot" : "mean";
        r.fields = c.fields;
        r.x = blocks[0]->nyGlobal, r.y = blocks[0]->nx, r.row0 = range.row0, r.rows = (long)range.rows();
        const std::size_t global = range.rows() * blocks[0]->nx;
        r.data.assign(c.fields.size() * global, 0.);
        forEachBlockInTurn(blocks, [&](DynamicsBlock& b) { // the blocks fill disjoint row ranges
            check(nsdg_ctx_synchronize(b.ctx.get()), "DynamicsStep: history flush");
            for (std::size_t k = 0; k < c.fields.size(); ++k)
                b.ownedRowsToHost(r.data.data() + k * global, range.row0, m_parts[b.index].acc + k * plane(b), false, "download history");
        });
        std::vector<double> weights;
        if (c.weighted()) { // the summed weights of the ice-weighted means, the same rows
            weights.assign(global, 0.);
            forEachBlockInTurn(blocks, [&](DynamicsBlock& b) { b.ownedRowsToHost(weights.data(), range.row0, m_parts[b.index].weight, false, "download history weights"); });
        }
        HistoryOutput::finish(c.stats, samples, global, weights.empty() ? nullptr : weights.data(), r.data);
        const RankEnvironment env = RankEnvironment::fromEnv(); // a process of a multi-process run writes its own rows
        HistoryOutput::write(HistoryOutput::recordPath(c.file, r.timeEnd, env.rank, env.world), c.file, r);
    }
    m_host.closeWindow();
}

// ------------------------------------------------------------------------------------------------ series
void SeriesChannel::allocate(DynamicsBlock& b)
{ // every slot is written before it is read: no memset
    m_parts[b.index] = b.outputBuffer((std::size_t)m_host.config().buffer * slotSize(b), "DynamicsStep: hipMalloc (series buffer)");
}

void SeriesChannel::afterStep(long dt, const DynamicsBlocks& blocks)
{ // the host counts the slots
    const std::vector<int>& ids = m_host.config().ids;
    const std::size_t slot = m_host.step(dt);
    forEachBlock(blocks, [&](DynamicsBlock& b) {
        const nsdg_history_sources src = b.sources(m_state.thermodynamics, m_state.advectColumn);
        check(nsdg_history_row_totals(b.ctx.get(), b.j0, b.j1, (int32_t)ids.size(), ids.data(), &src, SeriesOutput::EXTENT_CONC, b.j0, (int64_t)b.ownedRows(),
                  m_parts[b.index] + slot * slotSize(b)),
            "nsdg_history_row_totals");
    });
    if (m_host.full())
        atStop(blocks);
}

void SeriesChannel::atStop(const DynamicsBlocks& blocks)
{
    const SeriesOutput::Config& c = m_host.config();
    const std::size_t count = m_host.pending().size(), nq = c.ids.size();
    if (count == 0) // (a second stop())
        return;
    ScopedTimer timer("series flush");
    const RowRange range(blocks);
    const std::size_t nrows = range.rows();
    std::vector<double> rows(count * nq * nrows), part;
    forEachBlockInTurn(blocks, [&](DynamicsBlock& b) { // the blocks fill disjoint row ranges
        check(nsdg_ctx_synchronize(b.ctx.get()), "DynamicsStep: series flush");
        const std::size_t own = (std::size_t)b.ownedRows();
        part.resize(count * slotSize(b));
        toHost(part, m_parts[b.index], "download series");
        for (std::size_t s = 0; s < count * nq; ++s)
            std::copy(part.begin() + s * own, part.begin() + (s + 1) * own, rows.begin() + s * nrows + (b.r0 - range.row0));
    });
    const double hx = m_L / blocks[0]->nx, hy = m_L / blocks[0]->nyGlobal;
    std::vector<std::string> lines;
    for (std::size_t s = 0; s < count; ++s)
        lines.push_back(SeriesOutput::formatLine(m_host.pending()[s], SeriesOutput::totals(c.ids, rows.data() + s * nq * nrows, nrows, hx, hy)));
    SeriesOutput::append(c, lines);
    m_host.flushed();
}

// ------------------------------------------------------------------------------------------------ momentum budget
void BudgetChannel::allocate(DynamicsBlock& b)
{ // the launch writes the owned node rows and only they are read: no memset
    Part& p = m_parts[b.index];
    const BudgetOutput::Config& c = m_host.config();
    if (!c.file.empty())
        p.planes = b.outputBuffer(2 * c.ids.size() * (std::size_t)b.NN, "DynamicsStep: hipMalloc (budget planes)");
    if (!c.seriesFile.empty())
        p.power = b.outputBuffer((std::size_t)NSDG_BUDGET_QUANTITIES * b.ownedRows(), "DynamicsStep: hipMalloc (budget row totals)");
}

void BudgetChannel::launch(DynamicsBlock& b)
{
    const Part& p = m_parts[b.index];
    const std::vector<int>& ids = m_host.config().ids;
    nsdg_budget_out out = {};
    double** plane[NSDG_BUDGET_TERMS][2] = { { &out.wind_x, &out.wind_y }, { &out.water_x, &out.water_y }, { &out.coriolis_x, &out.coriolis_y },
        { &out.tilt_x, &out.tilt_y }, { &out.internal_x, &out.internal_y }, { &out.basal_x, &out.basal_y }, { &out.inertia_x, &out.inertia_y },
        { &out.residual_x, &out.residual_y } };
    if (p.planes)
        for (std::size_t k = 0; k < ids.size(); ++k)
            for (int c = 0; c < 2; ++c)
                *plane[ids[k]][c] = p.planes + (2 * k + c) * (std::size_t)b.NN;
    out.power = p.power, out.power_stride = b.ownedRows(), out.row0 = b.j0;
    // the current side of the ping-pongs: the stress and the velocity the sub-cycle left, H and A the transport has not moved yet
    const bool a = b.par == 0;
    check(nsdg_momentum_budget(b.ctx.get(), b.j0, b.j1, b.cur(FH), b.cur(FA), b.d[UA], b.d[VA], b.d[a ? S11a : S11b], b.d[a ? S12a : S12b],
              b.d[a ? S22a : S22b], b.curU(), b.curV(), b.d[PACKED], &out),
        "nsdg_momentum_budget");
}

void BudgetChannel::afterStep(long dt, const DynamicsBlocks& blocks)
{
    const bool record = m_host.step(dt);
    if (!m_host.config().seriesFile.empty()) {
        const RowRange range(blocks);
        const std::size_t nrows = range.rows();
        std::vector<double> rows(NSDG_BUDGET_QUANTITIES * nrows), part;
        forEachBlockInTurn(blocks, [&](DynamicsBlock& b) { // the blocks fill disjoint row ranges
            check(nsdg_ctx_synchronize(b.ctx.get()), "DynamicsStep: budget series");
            const std::size_t own = (std::size_t)b.ownedRows();
            part.resize(NSDG_BUDGET_QUANTITIES * own);
            toHost(part, m_parts[b.index].power, "download budget row totals");
            for (std::size_t q = 0; q < NSDG_BUDGET_QUANTITIES; ++q)
                std::copy(part.begin() + q * own, part.begin() + (q + 1) * own, rows.begin() + q * nrows + (b.r0 - range.row0));
        });
        m_host.appendLine(BudgetOutput::formatLine(m_host.clock(), BudgetOutput::totals(rows.data(), nrows)));
    }
    if (record)
        write(blocks);
}

void BudgetChannel::atStop(const DynamicsBlocks& blocks)
{
    if (m_host.dueAtStop()) // (stop() comes twice: nothing is written twice)
        write(blocks);
}

void BudgetChannel::write(const DynamicsBlocks& blocks)
{
    // a snapshot of the last (sub-)step: the owned node rows of every block into ONE host array per plane, with the history's record writer
    ScopedTimer timer("budget record");
    const BudgetOutput::Config& c = m_host.config();
    const RowRange range(blocks);
    const long nn = 2L * blocks[0]->nx + 1, nyg = blocks[0]->nyGlobal;
    const long rows = 2L * (long)range.rows() + (range.row1 == nyg ? 1 : 0);
    HistoryOutput::Record r;
    r.timeStart = r.timeEnd = m_host.clock(), r.samples = 1, r.kind = "snapshot";
    for (const std::string& t : c.terms)
        r.fields.push_back(t + "_x"), r.fields.push_back(t + "_y");
    r.x = 2 * nyg + 1, r.y = nn, r.row0 = 2L * range.row0, r.rows = rows;
    const std::size_t global = (std::size_t)(rows * nn);
    r.data.assign(r.fields.size() * global, 0.);
    forEachBlockInTurn(blocks, [&](DynamicsBlock& b) { // the blocks fill disjoint node rows
        check(nsdg_ctx_synchronize(b.ctx.get()), "DynamicsStep: budget record");
        const long own = 2L * b.ownedRows() + (b.r1 == nyg ? 1 : 0);
        for (std::size_t k = 0; k < r.fields.size(); ++k)
            checkHip(hipMemcpy(r.data.data() + k * global + 2L * (b.r0 - range.row0) * nn, m_parts[b.index].planes + k * (std::size_t)b.NN + 2L * b.j0 * nn,
                         (std::size_t)(own * nn) * sizeof(double), hipMemcpyDeviceToHost),
                "download budget planes");
    });
    HistoryOutput::write(HistoryOutput::recordPath(c.file, r.timeEnd), c.file, r);
}

// ------------------------------------------------------------------------------------------------ drifters
void DriftersChannel::allocate(DynamicsBlock& b)
{ // every block holds the whole list; the partner is written before it is read
    if (!any())
        return;
    Part& p = m_parts[b.index];
    for (double*& half : p.list)
        half = b.outputBuffer(m_list.size(), "DynamicsStep: hipMalloc (drifters)");
    checkHip(hipMemcpy(p.list[0], m_list.data(), m_list.size() * sizeof(double), hipMemcpyHostToDevice), "upload drifters");
    p.current = 0;
    if (samplesSize()) // written by the first step before anything reads it
        p.samples = b.outputBuffer(samplesSize(), "DynamicsStep: hipMalloc (drifter samples)");
}

void DriftersChannel::advance(DynamicsBlock& b, double dt)
{
    if (!any())
        return;
    // the drifters of the owned rows move with the velocity the sub-cycle left (its ghost node rows are complete: the mEVP plan's ghost
    // zones are (v k, v k - 1) deep, the brittle plan ends with the exchange of every node row: complete_nodes) and the concentration the
    // transport left; then the blocks' lists are merged.  No phase of its own: inside the span, before its end mark
    Part& p = m_parts[b.index];
    nsdg_ctx* ctx = b.ctx.get();
    const int64_t n = (int64_t)count();
    check(nsdg_drifters_advance(ctx, b.j0, b.j1, dt, m_host.config().minConc, n, b.curU(), b.curV(), b.cur(FA), p.list[p.current], p.list[1 - p.current]),
        "nsdg_drifters_advance");
    p.current = 1 - p.current;
    double* now = p.list[p.current];
    if (b.world > 1)
        check(nsdg_comm_max_f64_array(ctx, now, 3 * n), "nsdg_comm_max_f64_array");
    if (p.samples) {
        // model.drifters_fields: the merged list is sampled at its NEW positions from the state the step left -- every block the
        // points of its own rows, -inf for the others -- and one more maximum makes the whole table
        const std::vector<int>& ids = m_host.config().fieldIds;
        const nsdg_history_sources src = b.sources(m_state.thermodynamics, m_state.advectColumn);
        check(nsdg_points_sample(ctx, b.j0, b.j1, 2, n, now, now + n, (int32_t)ids.size(), ids.data(), &src, n, p.samples), "nsdg_points_sample");
        if (b.world > 1)
            check(nsdg_comm_max_f64_array(ctx, p.samples, (int64_t)ids.size() * n), "nsdg_comm_max_f64_array");
    }
}

void DriftersChannel::afterStep(long dt, const DynamicsBlocks& blocks)
{
    m_sampled = true;
    if (m_host.step(dt))
        write(blocks);
}

void DriftersChannel::atStop(const DynamicsBlocks& blocks)
{
    if (m_host.dueAtStop()) // (stop() comes twice: the iterator's, the restart file's)
        write(blocks);
}

void DriftersChannel::write(const DynamicsBlocks& blocks)
{
    // every block holds the same list after the merge: row block 0 writes
    std::vector<double> planes(m_list.size()), samples(samplesSize());
    if (any()) {
        DynamicsBlock& b = *blocks[0];
        const Part& p = m_parts[0];
        checkHip(hipSetDevice(b.device), "hipSetDevice");
        check(nsdg_ctx_synchronize(b.ctx.get()), "DynamicsStep: drifters output");
        toHost(planes, p.list[p.current], "download drifters");
        if (!samples.empty()) {
            if (!m_sampled) // nothing has sampled yet (a run of no step): the fields of the start positions are not known
                std::fill(samples.begin(), samples.end(), std::numeric_limits<double>::quiet_NaN());
            else
                toHost(samples, p.samples, "download drifter samples");
        }
    }
    m_host.write(planes, samples);
}

// ------------------------------------------------------------------------------------------------ stations
void StationsChannel::allocate(DynamicsBlock& b)
{ // every slot is written before it is read: no memset
    if (m_xy.empty())
        return;
    Part& p = m_parts[b.index];
    p.xy = b.outputBuffer(m_xy.size(), "DynamicsStep: hipMalloc (stations)");
    checkHip(hipMemcpy(p.xy, m_xy.data(), m_xy.size() * sizeof(double), hipMemcpyHostToDevice), "upload stations");
    p.samples = b.outputBuffer((std::size_t)m_host.config().buffer * slotSize(), "DynamicsStep: hipMalloc (station buffer)");
}

void StationsChannel::afterStep(long dt, const DynamicsBlocks& blocks)
{ // the host counts the slots
    const std::vector<int>& ids = m_host.config().ids;
    const std::size_t slot = m_host.step(dt);
    const int64_t n = (int64_t)(m_xy.size() / 2);
    if (n > 0)
        forEachBlock(blocks, [&](DynamicsBlock& b) {
            const nsdg_history_sources src = b.sources(m_state.thermodynamics, m_state.advectColumn);
            const Part& p = m_parts[b.index];
            check(nsdg_points_sample(b.ctx.get(), b.j0, b.j1, 2, n, p.xy, p.xy + n, (int32_t)ids.size(), ids.data(), &src, n, p.samples + slot * slotSize()),
                "nsdg_points_sample");
        });
    if (m_host.full())
        atStop(blocks);
}

void StationsChannel::atStop(const DynamicsBlocks& blocks)
{
    const std::size_t pending = m_host.pending().size();
    if (pending == 0) // (a second stop())
        return;
    ScopedTimer timer("stations flush");
    std::vector<double> table(pending * slotSize(), -std::numeric_limits<double>::infinity()), part(table.size());
    if (!table.empty())
        forEachBlockInTurn(blocks, [&](DynamicsBlock& b) {
            check(nsdg_ctx_synchronize(b.ctx.get()), "DynamicsStep: stations flush");
            toHost(part, m_parts[b.index].samples, "download stations");
            for (std::size_t i = 0; i < table.size(); ++i)
                table[i] = (part[i] > table[i] || part[i] != part[i]) ? part[i] : table[i]; // (a NaN sample is kept)
        });
    m_host.write(m_xy, table);
}

} // namespace Nextsim
