// bbo_tabular.hpp -- the Tabular row format of the reference (src/tabular.hpp:65-77, values at max_digits10):
// what print=True of the restart drivers and of BasinHopping writes to stdout.
#pragma once

#include <cstdio>
#include <string>
#include <vector>

namespace bbo {

inline std::string tabular_int(long v) { return std::to_string(v); }

inline std::string tabular_double(double v)
{
    char buf[64];
    snprintf(buf, sizeof(buf), "%.17g", v);
    return buf;
}

inline void tabular_row(const std::vector<int> &widths, const std::vector<std::string> &cells, bool header)
{
    int sum = 0;
    for (size_t i = 0; i < cells.size(); i++) {
        printf(" | %*s", widths[i], cells[i].c_str());
        sum += widths[i];
    }
    printf(" | \n");
    if (header)
        printf(" |%s| \n", std::string(sum + 3 * ((int) cells.size() - 1) + 2, '=').c_str());
    fflush(stdout);
}

} // namespace bbo
