/* Create-time validation of an AmdMapConfig, shared by the HIP operator
 * (arroyo_amd_map_create) and the CPU oracle (oracle_map_create) so the two
 * accept exactly the same programs.  `max_out` is the caller's output-column
 * limit (AMD_MAP_MAX_OUT, or less).
 *
 * Beyond the range checks, every register that is actually read -- `a` and
 * `b` of a binary op, `a` of NOT / I2F / F2I / IS_NULL / IS_NOT_NULL,
 * nothing for CONST, `a`, `b` and register `imm` of SELECT, every
 * out_reg[i], filter_reg -- must be an input register or the dst of an
 * earlier instruction: a register has no value before it is written.
 * Operand fields an op does not read keep the plain range check.
 *
 * SQL NULLs (null_semantics = 1, opcodes above FDIV) exist only for an
 * includer that defines AMD_MAP_CHECK_NULLABLE before this header: the HIP
 * operator.  Everyone else -- the oracle -- rejects null_semantics != 0
 * loudly, and opcodes above FDIV stay unknown in a null_semantics = 0
 * program either way. */
#ifndef ARROYO_AMD_MAP_CHECK_H
#define ARROYO_AMD_MAP_CHECK_H

#include "arroyo_amd_types.h"

/* NULL if the config is valid, else what is wrong with it */
static inline const char *amd_map_config_error(const AmdMapConfig *cfg,
                                               int max_out) {
    if (!cfg) return "null map config";
    if (cfg->n_in_cols < 1 || cfg->n_in_cols > AMD_MAP_MAX_REGS)
        return "invalid map config: n_in_cols out of range";
    if (cfg->n_prog < 0 || cfg->n_prog > AMD_MAP_MAX_PROG)
        return "invalid map config: n_prog out of range";
    if (cfg->n_out < 1 || cfg->n_out > max_out)
        return "invalid map config: n_out out of range";
    if (cfg->filter_reg < -1 || cfg->filter_reg >= AMD_MAP_MAX_REGS)
        return "invalid map config: filter_reg out of range";
    int max_op = AMD_MOP_FDIV;
#ifdef AMD_MAP_CHECK_NULLABLE
    if (cfg->null_semantics != 0 && cfg->null_semantics != 1)
        return "invalid map config: null_semantics must be 0 or 1";
    if (cfg->null_semantics) max_op = AMD_MOP_SELECT;
#else
    if (cfg->null_semantics != 0)
        return "invalid map config: null_semantics is not supported here";
#endif
    uint32_t written = cfg->n_in_cols == AMD_MAP_MAX_REGS
                           ? 0xffffffffu
                           : (1u << cfg->n_in_cols) - 1u;
    for (int i = 0; i < cfg->n_prog; i++) {
        const AmdMapInstr *in = &cfg->prog[i];
        if (in->op < AMD_MOP_CONST || in->op > max_op)
            return "invalid map program: unknown opcode";
        if (in->dst < 0 || in->dst >= AMD_MAP_MAX_REGS ||
            in->a < 0 || in->a >= AMD_MAP_MAX_REGS ||
            in->b < 0 || in->b >= AMD_MAP_MAX_REGS)
            return "invalid map program: register out of range";
        int reads_a = in->op != AMD_MOP_CONST;
        int reads_b = reads_a && in->op != AMD_MOP_NOT &&
                      in->op != AMD_MOP_I2F && in->op != AMD_MOP_F2I &&
                      in->op != AMD_MOP_IS_NULL &&
                      in->op != AMD_MOP_IS_NOT_NULL;
        if (in->op == AMD_MOP_SELECT) {
            if (in->imm < 0 || in->imm >= AMD_MAP_MAX_REGS)
                return "invalid map program: SELECT else-register (imm) "
                       "out of range";
            if (!(written >> in->imm & 1u))
                return "invalid map program: register read before it is "
                       "written";
        }
        if ((reads_a && !(written >> in->a & 1u)) ||
            (reads_b && !(written >> in->b & 1u)))
            return "invalid map program: register read before it is written";
        written |= 1u << in->dst;
    }
    for (int i = 0; i < cfg->n_out; i++) {
        if (cfg->out_reg[i] < 0 || cfg->out_reg[i] >= AMD_MAP_MAX_REGS)
            return "invalid map config: out_reg out of range";
        if (!(written >> cfg->out_reg[i] & 1u))
            return "invalid map config: out_reg is never written";
    }
    if (cfg->filter_reg >= 0 && !(written >> cfg->filter_reg & 1u))
        return "invalid map config: filter_reg is never written";
    return 0;
}

#endif /* ARROYO_AMD_MAP_CHECK_H */
