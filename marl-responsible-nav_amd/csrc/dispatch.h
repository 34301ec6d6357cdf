// dispatch.h — internal: the library's one switch over the agent count (gridenv.hip, actor_ops.hip).
#pragma once
#include <type_traits>

namespace gw {

// The kernels are templates of the agent count.  This is the only switch over it: f is a generic
// lambda called with std::integral_constant<int, N>; `bad` is the result for an N outside 1..8.
template <typename R, typename F>
R with_agents(int n, R bad, F &&f) {
    switch (n) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
    }
    return bad;
}

}  // namespace gw
